"""GPU tests of graph-level readout (run with -m gpu on an MI355X): ops.GraphBatch, ops.GraphClassifier and clf.on_batch.

The batch: 40 random graphs of 5 .. 60 vertices, one of 2 T + 9 vertices (a readout with chunk partials), one without edges and one of
a single vertex; dims [16, 32, 32], 3 classes.  A second batch of another vertex count serves on_batch.

Bars.  GraphBatch.from_graphs equals CsrGraph.from_coo on the hand-concatenated edge list.  For SageStack (mean, max), GcnStack (plain,
pad_streamed=True -- which pads nothing at these widths -- and, beyond the issue's list, dims [16, 72, 72] where the padded layout is
real and the readout pools a strided view) and GatStack, and each of the three pools: clf.train_step leaves the loss and EVERY
parameter of stack and head with the bits of the same step composed by hand from the public ops, and the pooled Z of clf.forward equals
tests/pool_ref.py on the host copy of net.forward(X) bit for bit.  A step through clf.on_batch(batch2) updates the same tensors, and a
step back on the first batch equals the hand-composed sequence again.

Learning.  The class of a graph is decided by the sign pattern of its mean feature in columns 0 and 1 (both negative / mixed / both
positive).  numpy_f64_loop below restates the SageStack(mean) + mean-pool classifier loop in float64 NumPy with the same initial
parameters; run on the CPU with LEARN_LR = 0.1 over 50 steps it gave loss 1.1496 at the first step and 0.1656 at the 50th (a fall to
14 %; accuracy 0.07 before the first step, 1.00 at the last; with 0.05 the fall is to 50 %, with 0.2 to 3 %), so the GPU assertion
"the 50th loss is below the first" has a wide margin."""
import importlib

import numpy as np
import pytest

from tests import pool_ref
from tests.helpers import synth
from tests.pool_ref import T

pytestmark = pytest.mark.gpu

DIMS, WIDE_DIMS, N_CLASSES = [16, 32, 32], [16, 72, 72], 3
LR, LEARN_LR, WD = 0.05, 0.1, 1e-3
POOLS = ("sum", "mean", "max")
# the SUM readout hands every vertex of a graph the graph's whole gradient and scales Z with the graph's size (up to 2 T + 9 here): its
# steps are taken 512 times smaller, or the second step already runs off to NaN (a matter of the optimisation, not of the wiring)
RATE = {"sum": LR / 512, "mean": LR, "max": LR}
STACKS = ("sage_mean", "sage_max", "gcn", "gcn_pad_streamed", "gcn_padded_wide", "gat")


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def make_graphs(seed, sizes):
    """[(src, dst, n)] int32 undirected edge lists (both directions, no duplicates, no self loops); a NEGATIVE size is a graph
    of that many vertices without edges."""
    rng = np.random.default_rng(seed)
    graphs = []
    for n in sizes:
        if n < 0 or n == 1:
            graphs.append((np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), abs(n)))
            continue
        pairs = set()
        for i in range(1, n):                                   # a spanning path's worth of edges plus random chords
            pairs.add((int(rng.integers(0, i)), i))
        for _ in range(n):
            a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
            if a != b:
                pairs.add((min(a, b), max(a, b)))
        e = np.array(sorted(pairs), dtype=np.int32)
        graphs.append((np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), n))
    return graphs


def make_task(seed, sizes):
    """graphs, features [n, 16] and the int32 class of each graph: the sign pattern of the graph's mean feature in columns 0 and 1."""
    graphs = make_graphs(seed, sizes)
    rng = np.random.default_rng(seed + 1)
    X, target = [], []
    for _, _, n in graphs:
        shift = np.zeros(DIMS[0])
        shift[:2] = rng.choice([-1.0, 1.0], size=2)
        x = (rng.standard_normal((n, DIMS[0])) + shift).astype(np.float32)
        m = x.astype(np.float64).mean(axis=0)
        X.append(x)
        target.append(int(m[0] > 0) + int(m[1] > 0))
    return graphs, np.concatenate(X), np.array(target, dtype=np.int32)


def sizes_one():
    rng = np.random.default_rng(3)
    return [int(v) for v in rng.integers(5, 61, size=40)] + [2 * T + 9, -7, 1]


def sizes_two():
    rng = np.random.default_rng(4)
    return [1, -3] + [int(v) for v in rng.integers(5, 61, size=25)] + [T + 3]


@pytest.fixture(scope="module")
def tasks(env):
    ops = env["ops"]
    out = []
    for seed, sizes in ((100, sizes_one()), (200, sizes_two())):
        graphs, X, target = make_task(seed, sizes)
        assert len(set(target.tolist())) == N_CLASSES
        batch = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, d), n) for s, d, n in graphs])
        # the wiring tests run on features scaled by 2^-6: the SUM readout of the 2 T + 9 vertex graph then stays small enough for the
        # loss kernel's -log(softmax) to be finite (a probability that underflows to 0 is an infinite loss, there as in the reference)
        out.append(dict(graphs=graphs, X=X, target=target, batch=batch, d_X=dev(env, X * np.float32(2.0 ** -6)), d_X_full=dev(env, X),
                        d_target=dev(env, target)))
    assert out[0]["batch"].n != out[1]["batch"].n and out[0]["batch"].n_graphs != out[1]["batch"].n_graphs
    return out


# ---- GraphBatch ------------------------------------------------------------------------------------------------------------------------------
def concatenated(graphs):
    ptr = np.concatenate([[0], np.cumsum([n for _, _, n in graphs])]).astype(np.int64)
    src = np.concatenate([s + off for (s, _, _), off in zip(graphs, ptr)]).astype(np.int32)
    dst = np.concatenate([d + off for (_, d, _), off in zip(graphs, ptr)]).astype(np.int32)
    return src, dst, ptr


def same_graph(a, b):
    for k in ("rowptr", "colidx", "rowptr_t", "colidx_t", "s", "norm"):
        x, y = host(getattr(a, k)), host(getattr(b, k))
        assert np.array_equal(bits(x), bits(y)), k
    assert a.n == b.n and a.nnz == b.nnz


def test_graph_batch_equals_the_hand_concatenated_graph(env, tasks):
    ops = env["ops"]
    t = tasks[0]
    src, dst, ptr = concatenated(t["graphs"])
    batch = t["batch"]
    assert isinstance(batch, ops.CsrGraph) and batch.nid is None
    same_graph(batch, ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), int(ptr[-1])))
    assert batch.n_graphs == len(t["graphs"]) and batch.graph_ptr.dtype == env["torch"].int32
    assert np.array_equal(host(batch.graph_ptr), ptr)
    assert batch.batch.dtype == env["torch"].int32
    assert np.array_equal(host(batch.batch), np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))
    lens = np.diff(ptr)
    assert (lens == 2 * T + 9).any() and (lens == 1).any() and lens.min() >= 1
    deg = np.diff(host(batch.rowptr))
    assert (deg[ptr[-3]:ptr[-2]] == 0).all() and deg[ptr[-2]] == 0               # the graph without edges and the single vertex
    two = ops.GraphBatch.from_coo_batched(dev(env, src), dev(env, dst), dev(env, ptr.astype(np.int32)))
    same_graph(batch, two)
    assert np.array_equal(host(two.graph_ptr), ptr) and two.n_graphs == batch.n_graphs
    no_t = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, d), n) for s, d, n in t["graphs"]], transpose=False, norm=False)
    assert no_t.rowptr_t is None and no_t.norm is None and np.array_equal(host(no_t.colidx), host(batch.colidx))


def test_from_graphs_refuses_an_edge_outside_its_graph(env, tasks):
    ops = env["ops"]
    graphs = [(s.copy(), d.copy(), n) for s, d, n in tasks[0]["graphs"][:4]]
    n0 = graphs[0][2]
    for a, b in ((n0, n0 + 1), (0, n0), (-1, 0)):              # both ends in the next graph's range; one end; a negative id
        bad = [(s.copy(), d.copy(), n) for s, d, n in graphs]
        bad[0][0][0], bad[0][1][0] = a, b
        with pytest.raises(ValueError):
            ops.GraphBatch.from_graphs([(dev(env, s), dev(env, d), n) for s, d, n in bad])
    ok = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, d), n) for s, d, n in graphs])
    assert ok.n_graphs == 4 and ok.n == sum(n for _, _, n in graphs)


def test_from_coo_batched_refuses_what_is_not_a_batch(env, tasks):
    ops = env["ops"]
    src, dst, ptr = concatenated(tasks[0]["graphs"])
    p32 = ptr.astype(np.int32)
    bad_src, bad_dst = src.copy(), dst.copy()
    bad_src[0], bad_dst[0] = ptr[1] - 1, ptr[1]                                   # the last vertex of graph 0 to the first of graph 1
    with pytest.raises(ValueError):
        ops.GraphBatch.from_coo_batched(dev(env, bad_src), dev(env, bad_dst), dev(env, p32))
    down = p32.copy()
    down[3], down[4] = down[4], down[3]
    assert down[4] < down[3]
    with pytest.raises(ValueError):
        ops.GraphBatch.from_coo_batched(dev(env, src), dev(env, dst), dev(env, down))
    with pytest.raises(ValueError):
        ops.GraphBatch.from_coo_batched(dev(env, src), dev(env, dst), dev(env, p32 + 1))      # does not start at 0
    with pytest.raises(ValueError):
        ops.GraphBatch.from_coo_batched(dev(env, src), dev(env, dst), dev(env, p32[:-3]))     # edges behind the last graph


# ---- wiring -------------------------------------------------------------------------------------------------------------------------------------
def make_net(env, kind, g, seed=5):
    ops = env["ops"]
    if kind.startswith("sage"):
        return ops.SageStack(g, DIMS, aggr=kind.split("_")[1], seed=seed)
    if kind == "gat":
        return ops.GatStack(g, DIMS, seed=seed)
    if kind == "gcn_padded_wide":
        net = ops.GcnStack(g, WIDE_DIMS, seed=seed, pad_streamed=True)
        assert net.padded
        return net
    return ops.GcnStack(g, DIMS, seed=seed, pad_streamed=(kind == "gcn_pad_streamed"))


PARAMS = {"SageStack": ("W_s", "W_n", "b"), "GatStack": ("W", "A", "b"), "GcnStack": ("Wp", "b")}
SHARED = {"SageStack": ("W_s", "W_n", "b", "dW_s", "dW_n", "db"), "GatStack": ("W", "A", "A_mask", "b", "dW", "dA", "db"),
          "GcnStack": ("Wp", "dWp", "W", "dW", "b", "db")}


def stack_params(net):
    return [p for name in PARAMS[type(net).__name__] for p in getattr(net, name)]


class ByHand:
    """The classifier's step composed from the public ops, on parameters of its own (drawn as GraphClassifier draws them)."""

    def __init__(self, env, kind, task, pool, seed=0):
        ops = env["ops"]
        self.env, self.kind, self.pool = env, kind, pool
        self.net = make_net(env, kind, task["batch"])
        d = self.net.dims[-1]
        self.W_c = dev(env, synth.uniform_pm1(seed + 1000, (N_CLASSES, d), scale=d ** -0.5))
        self.b_c = env["torch"].zeros(N_CLASSES, dtype=env["torch"].float32, device=env["dev"])
        self.db_c = env["torch"].zeros_like(self.b_c)
        assert ops is not None

    def rebound(self, task):
        """The same parameters under a stack built afresh on another batch: the constructor derives what it needs from the graph."""
        other = object.__new__(ByHand)
        other.__dict__.update(self.__dict__)
        other.net = make_net(self.env, self.kind, task["batch"])
        for name in SHARED[type(self.net).__name__]:
            setattr(other.net, name, getattr(self.net, name))
        return other

    def step(self, task, lr, wd):
        ops = self.env["ops"]
        ptr = task["batch"].graph_ptr
        H = self.net.forward(task["d_X"])
        Z, arg = ops.segment_pool(ptr, H, self.pool)
        logits = ops.bias_add(ops.gemm(Z, self.W_c, transB=True), self.b_c)
        loss, d = ops.softmax_ce(logits, task["d_target"], colsum_out=self.db_c)
        dW_c = ops.gemm(d, Z, transA=True)
        dZ = ops.gemm(d, self.W_c)
        dH = ops.segment_pool_bwd(ptr, dZ, self.pool, arg=arg, out=self.net.grad_buffer())
        self.net.backward(dH, input_grad=False)
        self.net.step(lr, wd)
        ops.sgd_step(self.W_c, dW_c, lr, wd)
        ops.sgd_step(self.b_c, self.db_c, lr, wd)
        return loss

    def params(self):
        return stack_params(self.net) + [self.W_c, self.b_c]


def clf_params(clf):
    return stack_params(clf.net) + [clf.W_c, clf.b_c]


def assert_same_params(clf, hand, what):
    for k, (a, b) in enumerate(zip(clf_params(clf), hand.params())):
        assert a.data_ptr() != b.data_ptr()
        assert np.array_equal(bits(host(a)), bits(host(b))), f"{what}: parameter {k}"


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("kind", STACKS)
def test_train_step_equals_the_step_composed_by_hand(env, tasks, kind, pool):
    ops = env["ops"]
    t = tasks[0]
    clf = ops.GraphClassifier(make_net(env, kind, t["batch"]), t["batch"], N_CLASSES, pool=pool)
    hand = ByHand(env, kind, t, pool)
    assert_same_params(clf, hand, "before")
    # the pooled Z of forward against the restatement on the host copy of the stack's output
    logits = clf.forward(t["d_X"])
    assert tuple(logits.shape) == (t["batch"].n_graphs, N_CLASSES) and tuple(clf.Z.shape) == (t["batch"].n_graphs, clf.net.dims[-1])
    H = np.ascontiguousarray(host(clf.net.forward(t["d_X"])))
    Zr, _ = pool_ref.pool_fwd(host(t["batch"].graph_ptr), H, pool)
    assert np.array_equal(bits(host(clf.Z)), bits(Zr))
    for k in range(2):
        before = [host(p).copy() for p in clf_params(clf)]
        loss = clf.train_step(t["d_X"], t["d_target"], RATE[pool], weight_decay=WD)
        loss_h = hand.step(t, RATE[pool], WD)
        assert np.isfinite(host(loss)).all() and np.array_equal(bits(host(loss)), bits(host(loss_h))), f"loss of step {k}"
        assert_same_params(clf, hand, f"step {k}")
        assert all((host(p) != b).any() for p, b in zip(clf_params(clf), before)), "a parameter did not move"
    ev_loss, correct, n = clf.evaluate(t["d_X"], t["d_target"])
    assert n == t["batch"].n_graphs and 0 <= correct <= n and np.isfinite(host(ev_loss)).all()


@pytest.mark.parametrize("kind,pool", list(zip(STACKS, ("mean", "max", "sum", "mean", "max", "sum"))))
def test_on_batch_shares_the_parameters_and_rebinds_the_graph(env, tasks, kind, pool):
    ops = env["ops"]
    t1, t2 = tasks
    net = make_net(env, kind, t1["batch"])
    clf = ops.GraphClassifier(net, t1["batch"], N_CLASSES, pool=pool)
    hand = ByHand(env, kind, t1, pool)
    clf2 = clf.on_batch(t2["batch"])
    hand2 = hand.rebound(t2)
    assert clf2.net.g is t2["batch"] and clf.net.g is t1["batch"] and clf2.net._saved is None
    for a, b in zip(clf_params(clf), clf_params(clf2)):
        assert a is b                                           # the SAME tensors
    assert clf2.dW_c is clf.dW_c and clf2.db_c is clf.db_c
    losses = []
    for c, h, t in ((clf, hand, t1), (clf2, hand2, t2), (clf, hand, t1)):
        before = [host(p).copy() for p in clf_params(clf)]
        loss, loss_h = c.train_step(t["d_X"], t["d_target"], RATE[pool], weight_decay=WD), h.step(t, RATE[pool], WD)
        assert np.array_equal(bits(host(loss)), bits(host(loss_h)))
        assert_same_params(clf, hand, f"{kind} after a step on a batch of {t['batch'].n} vertices")
        assert all((host(p) != b).any() for p, b in zip(clf_params(clf), before))
        losses.append(float(host(loss)[0]))
    assert all(np.isfinite(losses))


def test_sage_on_graph_still_refuses_another_vertex_count(env, tasks):
    ops = env["ops"]
    net = ops.SageStack(tasks[0]["batch"], DIMS)
    with pytest.raises(ValueError):
        net.on_graph(tasks[1]["batch"])


def test_classifier_arguments(env, tasks):
    ops = env["ops"]
    b = tasks[0]["batch"]
    net = ops.SageStack(b, DIMS)
    with pytest.raises(ValueError):
        ops.GraphClassifier(net, b, N_CLASSES, pool="min")
    g = ops.CsrGraph(b.n, b.rowptr, b.colidx, b.rowptr_t, b.colidx_t)
    with pytest.raises(TypeError):
        ops.GraphClassifier(net, g, N_CLASSES)
    # a stack built on another graph is bound to the classifier's batch
    clf = ops.GraphClassifier(ops.SageStack(tasks[1]["batch"], DIMS), b, N_CLASSES)
    assert clf.net.g is b and tuple(clf.forward(tasks[0]["d_X"]).shape) == (b.n_graphs, N_CLASSES)


# ---- learning ---------------------------------------------------------------------------------------------------------------------------------
def numpy_f64_loop(graphs, X, target, steps=50, lr=LEARN_LR, seed=5, head_seed=0):
    """SageStack(mean) + mean pool + linear head + softmax cross-entropy + SGD in float64 NumPy with dense matrices, from the same initial
    parameters; returns the loss of every step and the accuracy before the first and after the last."""
    src, dst, ptr = concatenated(graphs)
    n, B, L = int(ptr[-1]), len(graphs), len(DIMS) - 1
    A = np.zeros((n, n))
    A[src, dst] = 1.0
    np.fill_diagonal(A, 0.0)
    deg = A.sum(axis=1)
    A = A * np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)[:, None]            # M = inv_deg (.) (A h)
    P = np.zeros((B, n))
    for b in range(B):
        P[b, ptr[b]:ptr[b + 1]] = 1.0 / (ptr[b + 1] - ptr[b])
    W_s = [synth.uniform_pm1(seed + 2 * l, (DIMS[l + 1], DIMS[l]), scale=DIMS[l] ** -0.5).astype(np.float64) for l in range(L)]
    W_n = [synth.uniform_pm1(seed + 2 * l + 1, (DIMS[l + 1], DIMS[l]), scale=DIMS[l] ** -0.5).astype(np.float64) for l in range(L)]
    b_l = [np.zeros(DIMS[l + 1]) for l in range(L)]
    W_c = synth.uniform_pm1(head_seed + 1000, (N_CLASSES, DIMS[-1]), scale=DIMS[-1] ** -0.5).astype(np.float64)
    b_c = np.zeros(N_CLASSES)
    onehot = np.eye(N_CLASSES)[target]
    losses, accs = [], []
    for _ in range(steps):
        hs, Ms, h = [], [], X.astype(np.float64)
        for l in range(L):
            M = A @ h
            z = h @ W_s[l].T + M @ W_n[l].T + b_l[l]
            hs.append(h)
            Ms.append(M)
            h = np.maximum(z, 0.0) if l + 1 < L else z
        Z = P @ h
        logits = Z @ W_c.T + b_c
        logits -= logits.max(axis=1, keepdims=True)
        p = np.exp(logits)
        p /= p.sum(axis=1, keepdims=True)
        losses.append(float(-np.log(p[np.arange(B), target]).mean()))
        accs.append(float((p.argmax(axis=1) == target).mean()))
        d = (p - onehot) / B
        dW_c, db_c = d.T @ Z, d.sum(axis=0)
        G = P.T @ (d @ W_c)
        grads = []
        for l in reversed(range(L)):
            grads.append((l, G.T @ hs[l], G.T @ Ms[l], G.sum(axis=0)))
            if l:
                G = (G @ W_s[l] + A.T @ (G @ W_n[l])) * (hs[l] > 0)
        for l, gs, gn, gb in grads:
            W_s[l] -= lr * gs
            W_n[l] -= lr * gn
            b_l[l] -= lr * gb
        W_c -= lr * dW_c
        b_c -= lr * db_c
    return losses, accs[0], accs[-1]


def test_the_classifier_learns(env, tasks):
    ops = env["ops"]
    t = tasks[0]
    clf = ops.GraphClassifier(ops.SageStack(t["batch"], DIMS, aggr="mean", seed=5), t["batch"], N_CLASSES, pool="mean")
    losses = [float(host(clf.train_step(t["d_X_full"], t["d_target"], LEARN_LR))[0]) for _ in range(50)]
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0], (losses[0], losses[-1])
