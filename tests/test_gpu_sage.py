"""GPU tests of ops.SageStack (run with -m gpu on an MI355X) on the task of tests/test_gpu_gat.py: the R-MAT graph with N = 1024 and
E = 8000 as CsrGraph.from_coo builds it (isolated vertices: empty neighbourhoods), dims [16, 32, 16], every third row labelled; for
both aggregators.

Bars (none is new): the aggregated M of a layer -- and for max the saved arg -- bit for bit against the restatements (tests/spmm_ref.py
with rowscale = 1 / deg; tests/reduce_ref.py); the layer output within 1e-5 * max(1, |ref|) of float64; one whole step against a float64
autograd model at the bounds of test_gpu_gat.py::test_one_step_vs_float64 -- 1e-5 * max(1, |ref|) for the loss, 2e-5 * max(|ref|_max,
1e-3) for every parameter gradient.  For max the float64 model routes through the device's saved arg (a gather by colidx[arg], masked
where arg == -1), which makes the comparison differentiable and immune to near-ties; that the device's choice IS a float64 maximiser
within 1e-5 * max(1, |max|) is asserted separately.  Training goes down and repeats bit for bit."""
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests.helpers import synth
from tests.reduce_ref import spmm_reduce_ref
from tests.spmm_ref import spmm_ref

pytestmark = pytest.mark.gpu

N, E, DIMS = 1 << 10, 8000, [16, 32, 16]
LR = 0.05
AGGRS = ["mean", "max"]


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


@pytest.fixture(scope="module")
def task(env):
    ops = env["ops"]
    src, dst = synth.rmat_edges(91, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    g.make_plans(64, max(DIMS))
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    deg = np.diff(rowptr)
    assert (deg == 0).any() and deg.max() > 64
    inv_deg = np.where(deg > 0, np.float32(1) / np.maximum(deg, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32)
    rows = np.arange(0, N, 3, dtype=np.int32)
    return dict(g=g, src=src, dst=dst, rowptr=rowptr, colidx=colidx, deg=deg, inv_deg=inv_deg, X=X, target=target, rows=rows)


def make_net(env, g, aggr, dims=DIMS, seed=950):
    net = env["ops"].SageStack(g, dims, aggr=aggr, seed=seed)
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (dims[l + 1],), scale=0.2)))
    return net


@pytest.mark.parametrize("aggr", AGGRS)
def test_one_layer_forward(env, task, aggr):
    net = make_net(env, task["g"], aggr, dims=DIMS[:2])
    assert tuple(net.W_s[0].shape) == (DIMS[1], DIMS[0]) and tuple(net.W_n[0].shape) == (DIMS[1], DIMS[0])
    assert not env["torch"].equal(net.W_s[0], net.W_n[0])
    Z = host(net.forward(dev(env, task["X"])))
    h, M, arg, _ = net._saved[0]
    rp, ci, X = task["rowptr"], task["colidx"], task["X"]
    if aggr == "mean":
        assert np.array_equal(host(net.inv_deg), task["inv_deg"])
        M_ref = spmm_ref(rp, ci, X, rowscale=task["inv_deg"])
        assert arg is None
    else:
        M_ref, arg_ref = spmm_reduce_ref(rp, ci, X, None, "max")
        assert np.array_equal(host(arg), arg_ref)
    assert np.array_equal(host(M).view(np.int32), M_ref.view(np.int32))
    Ws, Wn, b = (host(t).astype(np.float64) for t in (net.W_s[0], net.W_n[0], net.b[0]))
    ref = X.astype(np.float64) @ Ws.T + M_ref.astype(np.float64) @ Wn.T + b
    assert (np.abs(Z - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()
    iso = np.nonzero(task["deg"] == 0)[0]      # an isolated vertex: h W_s^T + b
    assert (host(M)[iso] == 0).all()
    own = host(env["ops"].bias_add(env["ops"].gemm(dev(env, X), net.W_s[0], transB=True), net.b[0]))
    assert np.array_equal(Z[iso], own[iso])


def model64(torch, task, params, aggr, args):
    """The two-layer GraphSAGE and its loss in float64 autograd from float64 copies of the device's parameters; for max the winners are
    the device's (args[l]).  Returns (loss, per layer (float64 maximum, the chosen value))."""
    rows_e = torch.from_numpy(er.row_of_entries(task["rowptr"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    cols_pad = torch.cat([cols_e, torch.zeros(1, dtype=torch.int64)])
    inv_deg = torch.from_numpy(np.where(task["deg"] > 0, 1.0 / np.maximum(task["deg"], 1), 0.0))
    h = torch.from_numpy(task["X"].astype(np.float64))
    L = len(params["W_s"])
    chosen = []
    for l in range(L):
        F = h.shape[1]
        if aggr == "mean":
            M = torch.zeros((N, F), dtype=torch.float64).index_add(0, rows_e, h[cols_e]) * inv_deg[:, None]
        else:
            a = torch.from_numpy(args[l].astype(np.int64))                  # [N, F]; -1: an empty row
            src = cols_pad[a]                                                # -1 picks the pad
            M = torch.where(a >= 0, h.gather(0, src), torch.zeros((), dtype=torch.float64))
            true = torch.zeros((N, F), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, F), h.detach()[cols_e], "amax",
                                                                           include_self=False)
            chosen.append((true.numpy(), M.detach().numpy()))
        Z = h @ params["W_s"][l].T + M @ params["W_n"][l].T + params["b"][l]
        h = torch.relu(Z) if l + 1 < L else Z
    r = torch.from_numpy(task["rows"].astype(np.int64))
    tgt = torch.from_numpy(task["target"].astype(np.int64))[r]
    z = h[r]
    picked = z[torch.arange(len(r)), tgt]
    return (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r), chosen   # the loss kernel's form


@pytest.mark.parametrize("aggr", AGGRS)
def test_one_step_vs_float64(env, task, aggr):
    torch = env["torch"]
    net = make_net(env, task["g"], aggr)
    names = ("W_s", "W_n", "b")
    before = [p.clone() for k in names for p in getattr(net, k)]
    params = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in names}
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    args = [None if s[2] is None else host(s[2]) for s in net._saved]
    ref, chosen = model64(torch, task, params, aggr, args)
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"{aggr}: loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for l, (true, picked) in enumerate(chosen):          # the device's winner is a float64 maximiser
        gap = np.abs(true - picked) / np.maximum(1.0, np.abs(true))
        print(f"layer {l}: worst gap of the device's choice to the float64 maximum {gap.max():.3e}")
        assert (gap <= 1e-5).all()
        assert ((args[l] == -1) == (task["deg"] == 0)[:, None]).all()
    for l in range(len(net.W_s)):
        for got, r, nm in ((net.dW_s[l], params["W_s"][l].grad, f"dW_s{l}"), (net.dW_n[l], params["W_n"][l].grad, f"dW_n{l}"),
                           (net.db[l], params["b"][l].grad, f"db{l}")):
            got, r = host(got), r.numpy()
            err = np.abs(got - r).max()
            print(f"{nm}: err {err:.3e}, scale {np.abs(r).max():.3e}")
            assert np.abs(r).max() > 0
            assert err <= 2e-5 * max(np.abs(r).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(r).max():.3e}"
    for p, q in zip([p for k in names for p in getattr(net, k)], before):   # lr = 0: the parameters keep their bits
        assert torch.equal(p, q)


@pytest.mark.parametrize("aggr", AGGRS)
def test_training_goes_down_and_repeats_bit_for_bit(env, task, aggr):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    runs = []
    for _ in range(2):
        net = make_net(env, task["g"], aggr)
        losses = [float(host(net.train_step(X, t, rows, lr=LR))[0]) for _ in range(30)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.W_s + net.W_n + net.b]))
    print(f"{aggr}: loss {runs[0][0][0]:.4f} -> {runs[0][0][-1]:.4f}")
    assert runs[0][0] == runs[1][0]
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)
    loss, correct, count = make_net(env, task["g"], aggr).evaluate(X, t, rows)
    assert count == len(task["rows"]) and 0 <= correct <= count and np.isfinite(host(loss)[0])


def test_max_refuses_what_the_transpose_map_refuses(env, task):
    ops, capi = env["ops"], env["capi"]
    s, d = dev(env, task["src"]), dev(env, task["dst"])
    g = ops.CsrGraph.from_coo(s, d, N, relabel="scramble")
    with pytest.raises(capi.GnnxError, match="relabel"):
        ops.SageStack(g, DIMS, aggr="max")
    g2 = ops.CsrGraph.from_coo(s, d, N, transpose=False)
    with pytest.raises(capi.GnnxError, match="transposed"):
        ops.SageStack(g2, DIMS, aggr="max")
    with pytest.raises(ValueError):
        ops.SageStack(task["g"], DIMS, aggr="sum")


def test_mean_on_a_relabelled_graph_keeps_its_bits(env, task):
    """The aggregation's order survives relabelling: in vertex order, M of every layer and the logits carry the unrelabelled stack's bits."""
    ops, torch = env["ops"], env["torch"]
    g = ops.CsrGraph.from_coo(dev(env, task["src"]), dev(env, task["dst"]), N, relabel="scramble")
    g.make_plans(64, max(DIMS))
    assert g.nid is not None
    plain, moved = make_net(env, task["g"], "mean"), make_net(env, g, "mean")
    X = dev(env, task["X"])
    logits = plain.forward(X)
    logits_r = moved.forward(g.to_new_order(X))
    for l in range(len(DIMS) - 1):
        assert torch.equal(g.to_vertex_order(moved._saved[l][1]), plain._saved[l][1]), f"M{l}"
    assert torch.equal(g.to_vertex_order(logits_r), logits)
    assert np.array_equal(host(plain._saved[0][1]), spmm_ref(task["rowptr"], task["colidx"], task["X"], rowscale=task["inv_deg"]))


@pytest.mark.parametrize("aggr", AGGRS)
def test_each_layer_runs_the_kernels_it_should(env, task, aggr, monkeypatch):
    """Per layer and direction ONE aggregation: spmm_reduce / spmm_reduce_bwd for max, the PLANNED spmm on CSR(A) / CSR(A^T) for mean.
    A training step needs no input gradient: its backward skips layer 0's aggregation."""
    ops, g = env["ops"], task["g"]
    calls = []

    def record(name):
        inner = getattr(ops, name)

        def wrapper(*a, **kw):
            calls.append((name, kw.get("plan")))
            return inner(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)

    for name in ("spmm", "spmm_reduce", "spmm_reduce_bwd", "spmm_heads", "transpose"):
        record(name)
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    net = make_net(env, g, aggr)
    L = len(DIMS) - 1

    def seen(fn):
        del calls[:]
        fn()
        return list(calls)

    def count(s, name, plan=None):
        return sum(1 for c in s if c[0] == name and (plan is None or c[1] is plan))

    fwd = seen(lambda: net.forward(X))
    bwd = seen(lambda: net.backward(dev(env, synth.uniform_pm1(97, (N, DIMS[-1])))))
    step = seen(lambda: net.train_step(X, t, rows, lr=0.0))
    if aggr == "max":
        assert count(fwd, "spmm_reduce") == L and len(fwd) == L
        assert count(bwd, "spmm_reduce_bwd") == L and len(bwd) == L
        assert [c[0] for c in step] == ["spmm_reduce"] * L + ["spmm_reduce_bwd"] * (L - 1)
    else:
        assert count(fwd, "spmm", g.plan) == L and len(fwd) == L
        assert count(bwd, "spmm", g.plan_t) == L and len(bwd) == L
        assert [c[1] for c in step] == [g.plan] * L + [g.plan_t] * (L - 1) and count(step, "spmm") == 2 * L - 1
