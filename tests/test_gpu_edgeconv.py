"""GPU tests of ops.knn_graph, GraphBatch.of_points and ops.EdgeConvStack (run with -m gpu on an MI355X), at the bars of
tests/test_gpu_sage.py -- none is new: the aggregated M and the saved arg of a layer bit for bit against tests/reduce_ref.py on the device's
T = h W_n^T; the layer output within 1e-5 * max(1, |ref|) of float64; one whole step against a float64 autograd model that routes through
the device's graphs (net.graphs) and winners (arg): 1e-5 * max(1, |ref|) for the loss, 2e-5 * max(|ref|_max, 1e-3) for every parameter
gradient, and the device's winner a float64 maximiser within 1e-5.  The graphs themselves are compared with tests/knn_ref.py by equality.
The task: 8 clouds of 5 .. 40 points in 3-D, dims [3, 16, 8]."""
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import knn_ref as kr
from tests.helpers import synth
from tests.reduce_ref import spmm_reduce_ref

pytestmark = pytest.mark.gpu

SIZES = [5, 40, 17, 8, 23, 31, 12, 36]
DIMS = [3, 16, 8]
K = 4
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


@pytest.fixture(scope="module")
def task(env):
    ptr = kr.ptr_of(SIZES)
    n = int(ptr[-1])
    X = synth.uniform_pm1(71, (n, DIMS[0]))
    target = ((5 * np.arange(n) + 1) % DIMS[-1]).astype(np.int32)
    rows = np.arange(0, n, 2, dtype=np.int32)
    fixed = env["ops"].knn_graph(dev(env, X), K, dev(env, ptr))
    return dict(ptr=ptr, n=n, X=X, target=target, rows=rows, fixed=fixed)


def entries(rowptr, colidx):
    return sorted(zip(er.row_of_entries(rowptr).tolist(), colidx.tolist()))


def test_knn_graph(env):
    ops, torch = env["ops"], env["torch"]
    sizes = [1, 3, 4, 5, 9, 30, 0, 2]                 # one point; k points or fewer; more than k; an empty cloud
    ptr = kr.ptr_of(sizes)
    n = int(ptr[-1])
    X = kr.exact_points(3, n, 3)                      # ties everywhere
    g = ops.knn_graph(dev(env, X), K, dev(env, ptr))
    assert isinstance(g, ops.GraphBatch) and g.n == n and g.n_graphs == len(sizes) and np.array_equal(host(g.graph_ptr), ptr)
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    ref_idx, _ = kr.knn_ref(X, K, segptr=ptr, flags=kr.EXCLUDE_SELF)
    want_deg = np.repeat(np.minimum(np.array(sizes) - 1, K).clip(min=0), sizes)
    assert np.array_equal(np.diff(rowptr), want_deg) and rowptr[0] == 0 and g.nnz == int(want_deg.sum()) == colidx.size
    assert want_deg[0] == 0 and (want_deg[1:4] == 2).all() and (want_deg[4:8] == 3).all() and (want_deg[8:13] == K).all()
    owner = np.repeat(np.arange(len(sizes)), sizes)
    for i in range(n):
        row = colidx[rowptr[i]:rowptr[i + 1]]
        assert np.array_equal(row, ref_idx[i][ref_idx[i] >= 0]), i
        assert (np.diff(row) > 0).all() and i not in row and (owner[row] == owner[i]).all()     # ascending, loop-free, inside its cloud
    assert entries(host(g.rowptr_t), host(g.colidx_t)) == sorted((c, r) for r, c in entries(rowptr, colidx))
    map_t = host(g.attention_map())
    assert np.array_equal(colidx[map_t], er.row_of_entries(host(g.rowptr_t)))                # entry q of A^T is entry map_t[q] of A
    assert g.norm is not None and g.plan is None
    # with loops every row holds itself; without graph_ptr one cloud and a plain CsrGraph; no short row: the flattened idx itself
    gl = ops.knn_graph(dev(env, X), K, dev(env, ptr), loop=True, norm=False)
    rp, ci = host(gl.rowptr), host(gl.colidx)
    assert all(i in ci[rp[i]:rp[i + 1]] for i in range(n)) and gl.norm is None
    g1 = ops.knn_graph(dev(env, X), K, transpose=False)
    assert type(g1) is ops.CsrGraph and g1.rowptr_t is None
    idx1, _ = kr.knn_ref(X, K, flags=kr.EXCLUDE_SELF)
    assert np.array_equal(host(g1.rowptr), np.arange(n + 1) * K) and np.array_equal(host(g1.colidx), idx1.reshape(-1))
    # clouds of one point only: an edgeless graph, both CSRs empty, and the stack still runs on it
    lone = ops.knn_graph(dev(env, X[:3]), K, dev(env, kr.ptr_of([1, 1, 1])))
    assert lone.nnz == 0 and not host(lone.rowptr).any() and not host(lone.rowptr_t).any() and lone.attention_map().numel() == 0
    pts = ops.GraphBatch.of_points(dev(env, ptr))
    assert pts.nnz == 0 and pts.n == n and pts.n_graphs == len(sizes) and np.array_equal(host(pts.graph_ptr), ptr)
    assert np.array_equal(host(pts.batch), owner) and pts.graph_ptr.dtype == torch.int32
    with pytest.raises(ValueError):
        ops.GraphBatch.of_points([0, 3, 2])


def make_net(env, g, k, dims=DIMS, seed=950):
    net = env["ops"].EdgeConvStack(g, dims, k=k, seed=seed)
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (dims[l + 1],), scale=0.2)))
    return net


def bound_graph(env, task, k):
    return task["fixed"] if k is None else env["ops"].GraphBatch.of_points(dev(env, task["ptr"]))


@pytest.mark.parametrize("k", [None, K])
def test_one_layer_forward(env, task, k):
    ops = env["ops"]
    net = make_net(env, bound_graph(env, task, k), k, dims=DIMS[:2])
    X = task["X"]
    Y = host(net.forward(dev(env, X)))
    h, M, arg, _ = net._saved[0]
    gl = net.graphs[0]
    rp, ci = host(gl.rowptr), host(gl.colidx)
    if k is None:
        assert gl is task["fixed"]
    else:                                             # the layer's graph is the k-NN graph of its input, cloud by cloud
        ref_idx, _ = kr.knn_ref(X, K, segptr=task["ptr"], flags=kr.EXCLUDE_SELF)
        assert np.array_equal(ci, ref_idx[ref_idx >= 0]) and np.array_equal(np.diff(rp), (ref_idx >= 0).sum(1))
    T = host(ops.gemm(dev(env, X), net.W_n[0], transB=True))
    M_ref, arg_ref = spmm_reduce_ref(rp, ci, T, None, "max")
    assert np.array_equal(host(arg), arg_ref) and np.array_equal(host(M).view(np.int32), M_ref.view(np.int32))
    Ws, b = host(net.W_s[0]).astype(np.float64), host(net.b[0]).astype(np.float64)
    Wn = host(net.W_n[0]).astype(np.float64)
    T64 = X.astype(np.float64) @ Wn.T
    M64 = np.take_along_axis(T64, ci[np.maximum(arg_ref, 0)].astype(np.int64), 0) * (arg_ref >= 0)
    ref = X.astype(np.float64) @ Ws.T + M64 + b
    assert (np.abs(Y - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()


def model64(torch, task, params, graphs, args):
    """The two-layer stack and its loss in float64 autograd from float64 copies of the device's parameters, on the device's per-layer
    graphs with the device's winners.  Returns (loss, per layer (float64 maximum, the chosen value))."""
    h = torch.from_numpy(task["X"].astype(np.float64))
    n, L = task["n"], len(params["W_s"])
    chosen = []
    for l in range(L):
        rp, ci = graphs[l]
        rows_e = torch.from_numpy(er.row_of_entries(rp))
        cols_e = torch.from_numpy(ci.astype(np.int64))
        cols_pad = torch.cat([cols_e, torch.zeros(1, dtype=torch.int64)])
        T = h @ params["W_n"][l].T
        F = T.shape[1]
        a = torch.from_numpy(args[l].astype(np.int64))                  # [n, F]; -1: an empty row
        M = torch.where(a >= 0, T.gather(0, cols_pad[a]), torch.zeros((), dtype=torch.float64))
        true = torch.zeros((n, F), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, F), T.detach()[cols_e], "amax",
                                                                       include_self=False)
        chosen.append((true.numpy(), M.detach().numpy()))
        Z = h @ params["W_s"][l].T + M + params["b"][l]
        h = torch.relu(Z) if l + 1 < L else Z
    r = torch.from_numpy(task["rows"].astype(np.int64))
    tgt = torch.from_numpy(task["target"].astype(np.int64))[r]
    z = h[r]
    picked = z[torch.arange(len(r)), tgt]
    return (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r), chosen   # the loss kernel's form


@pytest.mark.parametrize("k", [None, K])
def test_one_step_vs_float64(env, task, k):
    torch = env["torch"]
    net = make_net(env, bound_graph(env, task, k), k)
    names = ("W_s", "W_n", "b")
    before = [p.clone() for nm in names for p in getattr(net, nm)]
    params = {nm: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, nm)] for nm in names}
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    assert len(net.graphs) == len(DIMS) - 1
    graphs = [(host(g.rowptr), host(g.colidx)) for g in net.graphs]
    if k is not None:                                  # layer 1's graph comes from layer 0's output: not the input's graph
        assert not np.array_equal(graphs[0][1], graphs[1][1])
        for rp, _ in graphs:
            assert np.array_equal(np.diff(rp), np.full(task["n"], K))          # every cloud has more than k points
    args = [host(s[2]) for s in net._saved]
    ref, chosen = model64(torch, task, params, graphs, args)
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"k={k}: loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for l, (true, picked) in enumerate(chosen):          # the device's winner is a float64 maximiser
        gap = np.abs(true - picked) / np.maximum(1.0, np.abs(true))
        print(f"layer {l}: worst gap of the device's choice to the float64 maximum {gap.max():.3e}")
        assert (gap <= 1e-5).all() and (args[l] >= 0).all()
    for l in range(len(net.W_s)):
        for got, r, nm in ((net.dW_s[l], params["W_s"][l].grad, f"dW_s{l}"), (net.dW_n[l], params["W_n"][l].grad, f"dW_n{l}"),
                           (net.db[l], params["b"][l].grad, f"db{l}")):
            got, r = host(got), r.numpy()
            err = np.abs(got - r).max()
            print(f"{nm}: err {err:.3e}, scale {np.abs(r).max():.3e}")
            assert np.abs(r).max() > 0
            assert err <= 2e-5 * max(np.abs(r).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(r).max():.3e}"
    for p, q in zip([p for nm in names for p in getattr(net, nm)], before):   # lr = 0: the parameters keep their bits
        assert torch.equal(p, q)


def test_input_gradient_and_on_graph(env, task):
    """backward returns dL/dX through both paths; on_graph shares parameters and buffers."""
    torch, ops = env["torch"], env["ops"]
    net = make_net(env, task["fixed"], None)
    X = dev(env, task["X"])
    out = net.forward(X)
    dOut = dev(env, synth.uniform_pm1(97, tuple(out.shape)))
    dX = host(net.backward(dOut))
    params = {nm: [torch.tensor(host(p).astype(np.float64)) for p in getattr(net, nm)] for nm in ("W_s", "W_n", "b")}
    x64 = torch.tensor(task["X"].astype(np.float64), requires_grad=True)
    g = task["fixed"]
    cols_pad = torch.cat([torch.from_numpy(host(g.colidx).astype(np.int64)), torch.zeros(1, dtype=torch.int64)])
    h = x64
    for l in range(len(DIMS) - 1):
        a = torch.from_numpy(host(net._saved[l][2]).astype(np.int64))
        T = h @ params["W_n"][l].T
        Z = h @ params["W_s"][l].T + torch.where(a >= 0, T.gather(0, cols_pad[a]), torch.zeros((), dtype=torch.float64)) + params["b"][l]
        h = torch.relu(Z) if l + 1 < len(DIMS) - 1 else Z
    (h * torch.from_numpy(host(dOut).astype(np.float64))).sum().backward()
    r = x64.grad.numpy()
    assert np.abs(dX - r).max() <= 2e-5 * max(np.abs(r).max(), 1e-3)
    other = ops.knn_graph(X, 2, dev(env, task["ptr"]))
    view = net.on_graph(other)
    assert view.W_s[0] is net.W_s[0] and view._buf is net._buf and view.g is other and net.g is task["fixed"]
    assert tuple(view.forward(X).shape) == tuple(out.shape) and view.graphs[0] is other and view.graphs[1] is other
    with pytest.raises(ValueError):
        net.on_graph(ops.GraphBatch.of_points(dev(env, kr.ptr_of([3, 4]))))


def test_classifier_trains_and_repeats_bit_for_bit(env, task):
    torch, ops = env["torch"], env["ops"]
    X = dev(env, task["X"])
    labels = dev(env, (np.arange(len(SIZES)) % 3).astype(np.int32))
    runs = []
    for _ in range(2):
        pts = ops.GraphBatch.of_points(dev(env, task["ptr"]))
        clf = ops.GraphClassifier(make_net(env, pts, K), pts, 3, pool="max", seed=5)
        assert isinstance(clf.net, ops.EdgeConvStack) and clf.net.k == K
        losses = [float(host(clf.train_step(X, labels, lr=LR))[0]) for _ in range(30)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in clf.params()], clf))
    print(f"loss {runs[0][0][0]:.4f} -> {runs[0][0][-1]:.4f}")
    assert runs[0][0] == runs[1][0]
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)
    clf = runs[0][2]
    # another batch size: the first three clouds; the same parameter tensors, and a step through the view moves them
    sub_ptr = task["ptr"][:4]
    sub = clf.on_batch(ops.GraphBatch.of_points(dev(env, sub_ptr)))
    assert all(a is b for a, b in zip(sub.params(), clf.params())) and sub.net.g.n == int(sub_ptr[-1]) and sub.net.k == K
    before = [p.clone() for p in clf.params()]
    loss = sub.train_step(X[:int(sub_ptr[-1])].contiguous(), labels[:3].contiguous(), lr=LR)
    assert np.isfinite(host(loss)[0]) and len(sub.net.graphs) == len(DIMS) - 1 and sub.net.graphs[0].n_graphs == 3
    assert any(not torch.equal(p, q) for p, q in zip(clf.params(), before))
    loss_e, correct, count = clf.evaluate(X, labels)
    assert count == len(SIZES) and 0 <= correct <= count and np.isfinite(host(loss_e)[0])
