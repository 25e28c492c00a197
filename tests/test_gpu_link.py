"""GPU tests of link prediction on ops.GcnStack (run with -m gpu on an MI355X): EdgeSet.from_pairs, link_scores, the gradient that
goes back through the pair scores to both endpoints, one step against a float64 model, and training.

Bars (none is new): bit equality against the NumPy restatements (tests/sddmm_ref.py for the scores, tests/spmm_ref.py for the two
aggregations that form dZ); the whole step against float64 at the bounds of test_gpu_parity.py::test_two_layer_training_step_vs_float64
-- 1e-5 * max(1, |ref|) for the loss, 2e-5 * max(|ref|_max, 1e-3) for the parameter gradients."""
import importlib

import numpy as np
import pytest

import oracle
from tests import sddmm_ref as sr
from tests.helpers import synth
from tests.spmm_ref import spmm_ref

pytestmark = pytest.mark.gpu

N, E, DIMS = 1 << 10, 8000, [16, 32, 16]
# The reference's factorised norm (graph.cpp:177-185) is not a normalising operator: on this graph (largest degree 231) embeddings of
# hub vertices reach the thousands and the first loss is in the hundreds.  A float64 run of the same model goes down monotonically
# at this rate (364 -> 24 in 30 steps) and at a tenth of it; at 1e-4 it oscillates.
LR = 1e-5


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
    """R-MAT graph of 2^10 vertices; positives = every second edge of its list; as many uniform negatives, listed BEFORE them."""
    ops = env["ops"]
    src, dst = synth.rmat_edges(91, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    pos_s, pos_d = src[::2], dst[::2]
    neg_s, neg_d = synth.rmat_edges(92, N, len(pos_s), a=0.25, b=0.25, c=0.25)
    ps = np.concatenate([neg_s, pos_s]).astype(np.int32)
    pd = np.concatenate([neg_d, pos_d]).astype(np.int32)
    label = np.concatenate([np.zeros(len(neg_s)), np.ones(len(pos_s))]).astype(np.float32)
    edges = ops.EdgeSet.from_pairs(dev(env, ps), dev(env, pd), dev(env, label), N)
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    rp, ci = oracle.coo_to_csr(src, dst, N)
    _, norm = oracle.degree_norm(rp, ci, N)
    return dict(g=g, edges=edges, X=X, src=src, dst=dst, pos=(pos_s, pos_d), neg=(neg_s, neg_d), rp=rp, ci=ci, norm=norm)


def make_net(env, task, seed=950):
    ops = env["ops"]
    net = ops.GcnStack(task["g"], DIMS, seed=seed)
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    return net


def test_edge_set_pattern_and_colliding_pairs(env, task):
    """The pattern is the set of distinct pairs in (row, column) order; a pair listed as a negative AND as a positive carries label 1
    (the last duplicate wins and the positives come last); explicit 0 labels stay as entries."""
    e = task["edges"]
    pos = set(zip(task["pos"][0].tolist(), task["pos"][1].tolist()))
    neg = set(zip(task["neg"][0].tolist(), task["neg"][1].tolist()))
    assert pos & neg, "the setup must contain a collision"
    rowptr, colidx, target = host(e.rowptr), host(e.colidx), host(e.target)
    pairs = list(zip(sr.row_of_entries(rowptr).tolist(), colidx.tolist()))
    assert pairs == sorted(pos | neg)
    want = np.array([1.0 if p in pos else 0.0 for p in pairs], dtype=np.float32)
    assert np.array_equal(target, want)
    assert (want == 0).sum() == len(neg - pos) > 0
    rowptr_t, colidx_t = sr.transpose_csr(rowptr, colidx, N)
    assert np.array_equal(host(e.rowptr_t), rowptr_t) and np.array_equal(host(e.colidx_t), colidx_t)
    assert np.array_equal(host(e.map_t), sr.transpose_map_ref(rowptr, colidx, rowptr_t, colidx_t))


def test_link_scores_and_score_gradient_bits(env, task):
    ops, torch = env["ops"], env["torch"]
    net, e = make_net(env, task), task["edges"]
    X = dev(env, task["X"])
    scores = net.link_scores(X, e)
    Z = net.forward(X)
    Zh = host(Z)
    rowptr, colidx = host(e.rowptr), host(e.colidx)
    assert np.array_equal(host(scores), sr.sddmm_ref(rowptr, colidx, Zh, Zh))
    loss, ds = ops.bce_logits(scores, e.target)
    dZ = net.link_grad(Z, e, ds)
    dsh = host(ds)
    first = spmm_ref(rowptr, colidx, Zh, vals=dsh)
    ref = spmm_ref(host(e.rowptr_t), host(e.colidx_t), Zh, vals=dsh[host(e.map_t)], y0=first)
    assert np.array_equal(host(dZ), ref)
    assert torch.equal(dZ, net.link_grad(Z, e, ds, out=torch.empty_like(dZ)))


def test_link_step_vs_float64(env, task):
    """Loss, dW and db of one step against a float64 NumPy model of the same network and decoder."""
    import scipy.sparse as sp
    ops = env["ops"]
    net, e = make_net(env, task), task["edges"]
    W = [host(w).astype(np.float64) for w in net.W]
    b = [host(v).astype(np.float64) for v in net.b]
    loss = net.link_train_step(dev(env, task["X"]), e, lr=0.0)       # lr = 0: the gradients stay, the parameters do not move
    rowptr, colidx, y = host(e.rowptr), host(e.colidx).astype(np.int64), host(e.target).astype(np.float64)
    rows = sr.row_of_entries(rowptr)
    A = sp.csr_matrix((np.ones(len(task["ci"])), task["ci"], task["rp"]), shape=(N, N))
    S = sp.diags(task["norm"].astype(np.float64)) @ A
    x0 = task["X"].astype(np.float64)
    z1 = S @ (x0 @ W[0].T) + b[0]
    y1 = np.maximum(z1, 0)
    Z = S @ (y1 @ W[1].T) + b[1]
    s = (Z[rows] * Z[colidx]).sum(1)
    loss_ref, g = sr.bce_logits_ref64(s, y)
    P = sp.csr_matrix((g / len(s), (rows, colidx)), shape=(N, N))
    dz2 = P @ Z + P.T @ Z
    dh2 = S.T @ dz2
    dW1, db1 = dh2.T @ y1, dz2.sum(0)
    dz1 = (dh2 @ W[1]) * (z1 > 0)
    dh1 = S.T @ dz1
    dW0, db0 = dh1.T @ x0, dz1.sum(0)
    got_loss = float(host(loss)[0])
    print(f"loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for got, ref, nm in ((net.dW[1], dW1, "dW1"), (net.db[1], db1, "db1"), (net.dW[0], dW0, "dW0"), (net.db[0], db0, "db0")):
        err = np.abs(host(got) - ref).max()
        print(f"{nm}: err {err:.3e}, scale {np.abs(ref).max():.3e}")
        assert err <= 2e-5 * max(np.abs(ref).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(ref).max():.3e}"
    for w, w0 in zip(net.W + net.b, W + b):
        assert np.array_equal(host(w).astype(np.float64), w0)


def test_link_training_goes_down_and_repeats_bit_for_bit(env, task):
    torch = env["torch"]
    X, e = dev(env, task["X"]), task["edges"]
    runs = []
    for _ in range(2):
        net = make_net(env, task)
        losses = [float(host(net.link_train_step(X, e, lr=LR))[0]) for _ in range(30)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.W + net.b]))
    assert runs[0][0] == runs[1][0]
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)
