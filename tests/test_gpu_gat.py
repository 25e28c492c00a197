"""GPU tests of ops.GatStack (run with -m gpu on an MI355X): the single-head graph-attention stack on the R-MAT graph of
tests/test_gpu_link.py, once as CsrGraph.from_coo builds it (the diagonal stripped, isolated vertices: empty softmax rows) and once
with the whole diagonal filled (the paper's self attention).

Bars (none is new): bit equality of the one-head stack, forward and backward, against the chain of the public single-head calls it
replaced, and the kernels each layer must run (the planned aggregation and sddmm for one head, the _heads calls for several);
bit equality of one layer against the chain of restatements -- alpha from the device's own ER and expf through
tests/edge_softmax_ref.py, then tests/spmm_ref.py with vals = alpha; one whole step against a float64 autograd model at the bounds of
test_gpu_parity.py::test_two_layer_training_step_vs_float64 -- 1e-5 * max(1, |ref|) for the loss, 2e-5 * max(|ref|_max, 1e-3) for every
parameter gradient; training goes down and repeats bit for bit."""
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests.helpers import synth
from tests.spmm_ref import spmm_ref

pytestmark = pytest.mark.gpu

N, E, DIMS = 1 << 10, 8000, [16, 32, 16]
LR = 0.05


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", params=["stripped", "filled"])
def task(env, request):
    ops, torch = env["ops"], env["torch"]
    src, dst = synth.rmat_edges(91, N, E)
    s, d = dev(env, src), dev(env, dst)
    if request.param == "stripped":
        g = ops.CsrGraph.from_coo(s, d, N)
    else:   # the docstring's recipe: every diagonal entry, both directions, the values discarded
        w = torch.ones(s.numel(), dtype=torch.float32, device=env["dev"])
        rp, ci, _ = ops.csr_from_coo_weighted(s, d, w, N, ops.DIAG_FILL)
        rp_t, ci_t, _ = ops.csr_from_coo_weighted(d, s, w, N, ops.DIAG_FILL)
        g = ops.CsrGraph(N, rp, ci, rp_t, ci_t)
    g.make_plans(64, max(DIMS))
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    deg = np.diff(rowptr)
    rows_e = er.row_of_entries(rowptr)
    if request.param == "stripped":
        assert (deg == 0).any() and not (rows_e == colidx).any()
    else:
        assert deg.min() >= 1 and int((rows_e == colidx).sum()) == N
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32)
    rows = np.arange(0, N, 3, dtype=np.int32)
    return dict(g=g, rowptr=rowptr, colidx=colidx, X=X, target=target, rows=rows, kind=request.param)


def make_net(env, task, dims=DIMS, seed=950):
    net = env["ops"].GatStack(task["g"], dims, seed=seed)
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (dims[l + 1],), scale=0.2)))
    return net


def test_one_layer_forward_bits(env, task):
    """forward == spmm_ref(vals = x / z) with x the device's own expf of the restated argument and z its restated row sum."""
    ops = env["ops"]
    net = make_net(env, task, dims=DIMS[:2])
    assert net.negative_slope == 0.2
    Y = net.forward(dev(env, task["X"]))
    _, H, ER, alpha, _ = net._saved[0]
    rp, ci = task["rowptr"], task["colidx"]
    g = task["g"]
    x_d, m_d, z_d = ops.edge_softmax(g.rowptr, g.colidx, rowterm=ER[:, 0], colterm=ER[:, 1], negative_slope=0.2, unnormalised=True, want_stats=True)
    ERh = host(ER)
    e = er.leaky(er.pre_activation(rp, ci, rowterm=ERh[:, 0], colterm=ERh[:, 1]), 0.2)
    arg, m = er.exp_argument(e, rp)
    assert np.array_equal(host(m_d), m)
    x = host(x_d)
    x64 = np.exp(arg.astype(np.float64))
    normal = x64 >= 2.0 ** -126
    assert (np.abs(x - x64)[normal] <= 2 * np.spacing(x64[normal].astype(np.float32))).all()
    z = er.row_sum_in_order(x, rp)
    assert np.array_equal(host(z_d), z)
    alpha_ref = er.edge_softmax_from_x(x, z, rp)
    assert np.array_equal(host(alpha.reshape(-1)), alpha_ref)
    assert np.array_equal(host(Y), spmm_ref(rp, ci, host(H), vals=alpha_ref, bias=host(net.b[0])))
    if task["kind"] == "stripped":   # an isolated vertex: the bias alone
        iso = np.nonzero(np.diff(rp) == 0)[0]
        assert np.array_equal(host(Y)[iso], np.broadcast_to(host(net.b[0]), (len(iso), DIMS[1])))


def model64(torch, task, params, slope):
    """The two-layer GAT and its loss in float64 autograd from float64 copies of the device's parameters."""
    rows_e = torch.from_numpy(er.row_of_entries(task["rowptr"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    h = torch.from_numpy(task["X"].astype(np.float64))
    L = len(params["W"])
    for l in range(L):
        H = h @ params["W"][l].T
        t = (H @ params["A"][l][0])[rows_e] + (H @ params["A"][l][1])[cols_e]
        e = torch.nn.functional.leaky_relu(t, slope)
        m = torch.full((N,), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows_e, e.detach(), "amax")
        x = torch.exp(e - m[rows_e])
        alpha = x / torch.zeros(N, dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        Y = torch.zeros((N, H.shape[1]), dtype=torch.float64).index_add(0, rows_e, alpha[:, None] * H[cols_e]) + params["b"][l]
        h = torch.relu(Y) if l + 1 < L else Y
    r = torch.from_numpy(task["rows"].astype(np.int64))
    tgt = torch.from_numpy(task["target"].astype(np.int64))[r]
    z = h[r]
    picked = z[torch.arange(len(r)), tgt]
    return (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r)   # the loss kernel's form (reference nn.cpp:442-453)


def test_one_step_vs_float64(env, task):
    torch = env["torch"]
    net = make_net(env, task)
    before = [p.clone() for p in net.W + net.A + net.b]
    params = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in ("W", "A", "b")}
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    ref = model64(torch, task, params, float(np.float32(0.2)))
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for l in range(len(net.W)):
        dA = host(net.dA[l])
        for got, r, nm in ((host(net.dW[l]), params["W"][l].grad.numpy(), f"dW{l}"), (dA[0], params["A"][l].grad.numpy()[0], f"da_l{l}"),
                           (dA[1], params["A"][l].grad.numpy()[1], f"da_r{l}"), (host(net.db[l]), params["b"][l].grad.numpy(), f"db{l}")):
            err = np.abs(got - r).max()
            print(f"{nm}: err {err:.3e}, scale {np.abs(r).max():.3e}")
            assert np.abs(r).max() > 0
            assert err <= 2e-5 * max(np.abs(r).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(r).max():.3e}"
    for p, q in zip(net.W + net.A + net.b, before):   # lr = 0: the parameters keep their bits
        assert torch.equal(p, q)


def test_training_goes_down_and_repeats_bit_for_bit(env, task):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    runs = []
    for _ in range(2):
        net = make_net(env, task)
        losses = [float(host(net.train_step(X, t, rows, lr=LR))[0]) for _ in range(30)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.W + net.A + net.b]))
    print(f"loss {runs[0][0][0]:.4f} -> {runs[0][0][-1]:.4f}")
    assert runs[0][0] == runs[1][0]
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)
    loss, correct, count = make_net(env, task).evaluate(X, t, rows)
    assert count == len(task["rows"]) and 0 <= correct <= count and np.isfinite(host(loss)[0])


def test_one_head_stack_equals_the_chain_of_single_head_calls_bit_for_bit(env, task, monkeypatch):
    """GatStack(heads=None) runs its softmax and row sums on the multi-head calls with H = 1 and writes del / der straight into the
    halves of dER.  Every layer, forward and backward, restated from its saved (h, H, ER, alpha, Y) out of the public single-head
    wrappers (edge_softmax, the planned spmm, spmm_vals_grad, edge_softmax_bwd, csr_rowsum, the products) must give the same bits."""
    torch, ops, g = env["torch"], env["ops"], task["g"]
    for rowptr in (task["rowptr"], host(g.rowptr_t)):   # the planned kernel's split rows run in A and in A^T
        assert np.diff(rowptr).max() > 64
    assert g.plan is not None and g.plan_t is not None
    handed_down = []
    inner = ops.gemm_relu_colsum

    def recording(*a, **kw):
        out = inner(*a, **kw)
        handed_down.append(out[0])
        return out

    net = make_net(env, task)
    L = len(net.W)
    dOut = dev(env, synth.uniform_pm1(97, (N, DIMS[-1])))
    net.forward(dev(env, task["X"]))
    monkeypatch.setattr(ops, "gemm_relu_colsum", recording)
    dX = net.backward(dOut)
    monkeypatch.setattr(ops, "gemm_relu_colsum", inner)
    assert len(handed_down) == L - 1
    map_t = net.map_t.long()
    G = dOut
    assert torch.equal(net.db[L - 1], ops.colsum(G))
    for l in reversed(range(L)):
        h, H, ER, alpha, Y = net._saved[l]
        assert tuple(ER.shape) == (N, 2) and tuple(alpha.shape) == (g.nnz, 1)
        a = ops.edge_softmax(g.rowptr, g.colidx, rowterm=ER[:, 0], colterm=ER[:, 1], negative_slope=0.2)
        assert torch.equal(alpha.reshape(-1), a), f"alpha{l}"
        assert torch.equal(Y, ops.spmm(g.rowptr, g.colidx, H, vals=a, bias=net.b[l], plan=g.plan, relu_out=l + 1 < L)), f"Y{l}"
        dalpha = ops.spmm_vals_grad(g.rowptr, g.colidx, G, H)
        dt, d_el = ops.edge_softmax_bwd(g.rowptr, g.colidx, a, dalpha, rowterm=ER[:, 0], colterm=ER[:, 1], negative_slope=0.2)
        d_er = ops.csr_rowsum(g.rowptr_t, dt[map_t].contiguous())
        dH = ops.spmm(g.rowptr_t, g.colidx_t, G, vals=a[map_t].contiguous(), plan=g.plan_t)
        dER = torch.stack([d_el, d_er], dim=1).contiguous()
        ops.gemm(dER, net.A[l], out=dH, beta=1.0)
        assert torch.equal(net.dA[l], ops.gemm(dER, H, transA=True)), f"dA{l}"
        assert torch.equal(net.dW[l], ops.gemm(dH, h, transA=True)), f"dW{l}"
        if l == 0:
            G = ops.gemm(dH, net.W[0])
            assert torch.equal(dX, G), "dX"
        else:
            G, db = ops.gemm_relu_colsum(dH, net.W[l], h)
            assert torch.equal(handed_down[L - 1 - l], G), f"G{l - 1}"
            assert torch.equal(net.db[l - 1], db), f"db{l - 1}"


def test_each_layer_runs_the_kernels_it_should(env, task, monkeypatch):
    """The speed contract of the one layer path, which bit equality cannot see: a one-head layer aggregates on the PLANNED single-head
    kernel in both directions and takes its value gradient from sddmm; a layer of several heads runs the _heads calls; nothing is
    transposed."""
    ops, g = env["ops"], task["g"]
    calls = []

    def record(name):
        inner = getattr(ops, name)

        def wrapper(*a, **kw):
            calls.append((name, kw.get("plan")))
            return inner(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)

    for name in ("spmm", "spmm_heads", "sddmm", "sddmm_heads", "transpose"):
        record(name)
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])

    def step(heads):
        net = env["ops"].GatStack(g, DIMS, seed=950, heads=heads)
        del calls[:]
        net.train_step(X, t, rows, lr=0.0)
        return list(calls)

    def count(seen, name):
        return sum(1 for c in seen if c[0] == name)

    seen = step(None)                     # two one-head layers
    plans = [p for name, p in seen if name == "spmm"]
    assert len(plans) == 4 and sum(p is g.plan for p in plans) == 2 and sum(p is g.plan_t for p in plans) == 2
    assert count(seen, "sddmm") == 2
    assert count(seen, "spmm_heads") == 0 and count(seen, "sddmm_heads") == 0 and count(seen, "transpose") == 0
    seen = step([4, 1])                   # a 4-head layer under a one-head layer
    plans = [p for name, p in seen if name == "spmm"]
    assert len(plans) == 2 and sum(p is g.plan for p in plans) == 1 and sum(p is g.plan_t for p in plans) == 1
    assert count(seen, "sddmm") == 1
    assert count(seen, "spmm_heads") == 2 and count(seen, "sddmm_heads") == 1 and count(seen, "transpose") == 0
    # per layer: forward runs layer 0 then 1, backward 1 then 0 -- the 4-head layer's calls are the first and the last three
    order = [name for name, _ in seen]
    assert order == ["spmm_heads", "spmm", "sddmm", "spmm", "sddmm_heads", "spmm_heads"]


def test_relabelled_graph_is_refused(env):
    ops, capi = env["ops"], env["capi"]
    src, dst = synth.rmat_edges(91, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N, relabel="scramble")
    with pytest.raises(capi.GnnxError, match="relabel"):
        g.attention_map()
    with pytest.raises(capi.GnnxError, match="relabel"):
        ops.GatStack(g, DIMS)
    g2 = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N, transpose=False)
    with pytest.raises(capi.GnnxError, match="transposed"):
        g2.attention_map()
