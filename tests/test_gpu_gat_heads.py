"""GPU tests of ops.GatStack(heads=...) (run with -m gpu on an MI355X): the multi-head graph-attention stack on the graph of
tests/test_gpu_gat.py, once with the diagonal stripped (isolated vertices: empty softmax rows) and once filled.

Bars (those of tests/test_gpu_gat.py): bit equality of one layer against the chain of restatements -- alpha from the device's own ER and
expf through tests/heads_ref.py, then heads_ref.spmm_heads_ref with vals = alpha; one whole step against a float64 autograd model at
1e-5 * max(1, |ref|) for the loss and 2e-5 * max(|ref|_max, 1e-3) for every parameter gradient; heads = [1, 1] against heads = None bit for
bit; training goes down and repeats bit for bit."""
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import heads_ref as hr
from tests.helpers import synth

pytestmark = pytest.mark.gpu

N, E, DIMS, HEADS = 1 << 10, 8000, [16, 32, 16], [4, 1]
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
    else:
        w = torch.ones(s.numel(), dtype=torch.float32, device=env["dev"])
        rp, ci, _ = ops.csr_from_coo_weighted(s, d, w, N, ops.DIAG_FILL)
        rp_t, ci_t, _ = ops.csr_from_coo_weighted(d, s, w, N, ops.DIAG_FILL)
        g = ops.CsrGraph(N, rp, ci, rp_t, ci_t)
    g.make_plans(64, max(DIMS))
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    assert ((np.diff(rowptr) == 0).any()) == (request.param == "stripped")
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32)
    rows = np.arange(0, N, 3, dtype=np.int32)
    return dict(g=g, rowptr=rowptr, colidx=colidx, X=X, target=target, rows=rows, kind=request.param)


def make_net(env, task, dims=DIMS, heads=HEADS, seed=950):
    net = env["ops"].GatStack(task["g"], dims, seed=seed, heads=heads)
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (dims[l + 1],), scale=0.2)))
    return net


def test_one_layer_forward_bits(env, task):
    """forward == spmm_heads_ref(vals = x / z) with x the device's own expf of the restated argument and z its restated row sums."""
    ops = env["ops"]
    Hh = 4
    net = make_net(env, task, dims=DIMS[:2], heads=[Hh])
    Y = net.forward(dev(env, task["X"]))
    _, H, ER, alpha, _ = net._saved[0]
    assert tuple(ER.shape) == (N, 2 * Hh) and tuple(alpha.shape) == (len(task["colidx"]), Hh)
    A = host(net.A[0])
    assert np.array_equal(A != 0, host(net.A_mask[0]) != 0)
    rp, ci, g = task["rowptr"], task["colidx"], task["g"]
    x_d, m_d, z_d = ops.edge_softmax_heads(g.rowptr, g.colidx, Hh, rowterm=ER[:, :Hh], colterm=ER[:, Hh:], negative_slope=0.2, unnormalised=True,
                                           want_stats=True)
    ERh = host(ER)
    e = er.leaky(hr.pre_activation_heads(rp, ci, rowterm=ERh[:, :Hh], colterm=ERh[:, Hh:]), 0.2)
    arg, m = hr.exp_argument_heads(e, rp)
    assert np.array_equal(host(m_d), m)
    x = host(x_d)
    x64 = np.exp(arg.astype(np.float64))
    normal = x64 >= 2.0 ** -126
    assert (np.abs(x - x64)[normal] <= 2 * np.spacing(x64[normal].astype(np.float32))).all()
    z = hr.row_sum_in_order_heads(x, rp)
    assert np.array_equal(host(z_d), z)
    alpha_ref = hr.edge_softmax_heads_from_x(x, z, rp)
    assert np.array_equal(host(alpha), alpha_ref)
    assert np.array_equal(host(Y), hr.spmm_heads_ref(rp, ci, host(H), alpha_ref, Hh, bias=host(net.b[0])))
    if task["kind"] == "stripped":   # an isolated vertex: the bias alone
        iso = np.nonzero(np.diff(rp) == 0)[0]
        assert np.array_equal(host(Y)[iso], np.broadcast_to(host(net.b[0]), (len(iso), DIMS[1])))


def model64(torch, task, params, heads, slope):
    """The multi-head GAT and its loss in float64 autograd from float64 copies of the device's parameters (A the [2 Hh, Hh D] matrix)."""
    rows_e = torch.from_numpy(er.row_of_entries(task["rowptr"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    nnz = len(cols_e)
    h = torch.from_numpy(task["X"].astype(np.float64))
    L = len(params["W"])
    for l in range(L):
        Hh = heads[l]
        H = h @ params["W"][l].T
        ER = H @ params["A"][l].T
        t = ER[rows_e, :Hh] + ER[cols_e, Hh:]
        e = torch.nn.functional.leaky_relu(t, slope)
        m = torch.full((N, Hh), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, Hh), e.detach(), "amax")
        x = torch.exp(e - m[rows_e])
        alpha = x / torch.zeros((N, Hh), dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        msg = alpha[:, :, None] * H[cols_e].view(nnz, Hh, -1)
        Y = torch.zeros((N, Hh, msg.shape[2]), dtype=torch.float64).index_add(0, rows_e, msg).reshape(N, -1) + params["b"][l]
        h = torch.relu(Y) if l + 1 < L else Y
    r = torch.from_numpy(task["rows"].astype(np.int64))
    tgt = torch.from_numpy(task["target"].astype(np.int64))[r]
    z = h[r]
    picked = z[torch.arange(len(r)), tgt]
    return (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r)   # the loss kernel's form


def test_one_step_vs_float64(env, task):
    torch = env["torch"]
    net = make_net(env, task)
    before = [p.clone() for p in net.W + net.A + net.b]
    params = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in ("W", "A", "b")}
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    ref = model64(torch, task, params, HEADS, float(np.float32(0.2)))
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for l in range(len(net.W)):
        mask = host(net.A_mask[l]) != 0
        dA = host(net.dA[l])
        assert (dA[~mask] == 0).all(), "an entry of dA outside the blocks"
        dA_ref = np.where(mask, params["A"][l].grad.numpy(), 0.0)   # the blocks are the parameters
        for got, r, nm in ((host(net.dW[l]), params["W"][l].grad.numpy(), f"dW{l}"), (dA, dA_ref, f"dA{l}"),
                           (host(net.db[l]), params["b"][l].grad.numpy(), f"db{l}")):
            err = np.abs(got - r).max()
            print(f"{nm}: err {err:.3e}, scale {np.abs(r).max():.3e}")
            assert np.abs(r).max() > 0
            assert err <= 2e-5 * max(np.abs(r).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(r).max():.3e}"
    for p, q in zip(net.W + net.A + net.b, before):   # lr = 0: the parameters keep their bits
        assert torch.equal(p, q)


def test_single_heads_equal_the_single_head_stack_bit_for_bit(env, task):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    one, none = make_net(env, task, heads=[1, 1]), make_net(env, task, heads=None)
    for p, q in zip(one.W + one.A + one.b, none.W + none.A + none.b):
        assert torch.equal(p, q)
    l1, l0 = one.train_step(X, t, rows, lr=0.0), none.train_step(X, t, rows, lr=0.0)
    assert torch.equal(l1, l0)
    for nm, p, q in zip("W" * 2 + "A" * 2 + "b" * 2, one.dW + one.dA + one.db, none.dW + none.dA + none.db):
        assert torch.equal(p, q), f"d{nm}"
    for _ in range(30):
        assert torch.equal(one.train_step(X, t, rows, lr=LR), none.train_step(X, t, rows, lr=LR))
    for p, q in zip(one.W + one.A + one.b, none.W + none.A + none.b):
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
    net = make_net(env, task)
    for _ in range(3):
        net.train_step(X, t, rows, lr=LR)
    for l, A in enumerate(net.A):   # the step never leaves the blocks
        assert (host(A)[host(net.A_mask[l]) == 0] == 0).all()
    loss, correct, count = net.evaluate(X, t, rows)
    assert count == len(task["rows"]) and 0 <= correct <= count and np.isfinite(host(loss)[0])


def test_bad_heads_are_refused(env, task):
    ops = env["ops"]
    for heads in ([4], [4, 1, 1], [3, 1], [4, 0], [4, 1.5]):
        with pytest.raises(ValueError):
            ops.GatStack(task["g"], DIMS, heads=heads)
