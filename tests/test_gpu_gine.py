"""GPU tests of ops.GineStack (run with -m gpu on an MI355X): a 2-layer stack, dims [8, 16, 4], edge_dim 3, on a batch of three graphs
with n = 60 vertices and about 3 stored entries a row (duplicate edges and self loops in the list: their attribute rows get no gradient).

Bars (none is new; tests/test_gpu_sage.py uses them at the same depth): one train_step against a float64 autograd model on the CPU
within 1e-5 * max(1, |ref|) for the loss and 2e-5 * max(|ref|_max, 1e-3) for every parameter gradient, W_e and b_e included; the logits of
GraphClassifier, and of on_batch on a batch of another size, within the first bar.  Before comparing, no ReLU pre-activation of the float64
model may lie within 1e-5 of zero (the fixed seeds were checked on the CPU).  Twenty steps lower the loss and repeat bit for bit."""
import numpy as np
import pytest

from tests.helpers import synth
from tests.test_gpu_sage import dev, env, host  # noqa: F401

pytestmark = pytest.mark.gpu

DIMS, EDGE_DIM, SEED = [8, 16, 4], 3, 4100
NAMES = ("W_e", "W_1", "W_2", "b_e", "b_1", "b")


def make_task(env, sizes, seed):
    """A GraphBatch of len(sizes) graphs with 3 n_k listed edges each and its attributes; the host copies the float64 model reads."""
    ops = env["ops"]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    parts = [synth.uniform_edges(seed + k, n_k, 3 * n_k) for k, n_k in enumerate(sizes)]
    src = np.concatenate([s + o for (s, _), o in zip(parts, ptr)]).astype(np.int32)
    dst = np.concatenate([d + o for (_, d), o in zip(parts, ptr)]).astype(np.int32)
    n, attr = int(ptr[-1]), synth.uniform_pm1(seed + 50, (len(src), EDGE_DIM))
    g = ops.GraphBatch.from_coo_batched(dev(env, src), dev(env, dst), dev(env, ptr)).set_edge_attr(dev(env, src), dev(env, dst), dev(env, attr))
    rowptr, colidx = host(g.rowptr).astype(np.int64), host(g.colidx).astype(np.int64)
    last = {(s, d): x for x, (s, d) in enumerate(zip(src, dst))}        # of duplicate edges the last
    rows_e = np.repeat(np.arange(n), np.diff(rowptr))
    entry_edge = np.array([last[(r, c)] for r, c in zip(rows_e, colidx)])
    assert np.array_equal(host(g.entry_edge), entry_edge) and len(colidx) < len(src) and (src == dst).any()
    return dict(g=g, n=n, ptr=ptr, rows_e=rows_e, colidx=colidx, entry_edge=entry_edge, attr=attr, X=synth.uniform_pm1(seed + 51, (n, DIMS[0])),
                target=((5 * np.arange(n) + 1) % DIMS[-1]).astype(np.int32), rows=np.arange(0, n, 3, dtype=np.int32))


@pytest.fixture(scope="module")
def task(env):
    return make_task(env, (20, 25, 15), 70)


def make_net(env, g):
    net = env["ops"].GineStack(g, DIMS, EDGE_DIM, seed=SEED)
    for k, name in enumerate(("b_e", "b_1", "b")):
        for l, b in enumerate(getattr(net, name)):
            b.copy_(dev(env, synth.uniform_pm1(SEED + 100 + 10 * k + l, tuple(b.shape), scale=0.2)))
    return net


def model64(torch, t, P):
    """(h [n, dims[-1]], the smallest |ReLU pre-activation|) of the float64 stack on float64 copies P of the device's parameters."""
    rows_e, cols, ee = (torch.from_numpy(t[k]) for k in ("rows_e", "colidx", "entry_edge"))
    h, attr, margin = torch.from_numpy(t["X"].astype(np.float64)), torch.from_numpy(t["attr"].astype(np.float64)), np.inf
    L = len(P["W_1"])
    for l in range(L):
        m = h[cols] + (attr @ P["W_e"][l].T + P["b_e"][l])[ee]
        U = h + torch.zeros_like(h).index_add(0, rows_e, torch.relu(m))
        Z = U @ P["W_1"][l].T + P["b_1"][l]
        Y = torch.relu(Z) @ P["W_2"][l].T + P["b"][l]
        margin = min([margin, float(m.detach().abs().min()), float(Z.detach().abs().min())] + ([float(Y.detach().abs().min())] if l + 1 < L else []))
        h = torch.relu(Y) if l + 1 < L else Y
    return h, margin


def params64(torch, net, names=NAMES):
    return {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in names}


def test_one_step_vs_float64(env, task):
    torch = env["torch"]
    net = make_net(env, task["g"])
    P = params64(torch, net)
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    h, margin = model64(torch, task, P)
    assert margin > 1e-5, margin
    r = torch.from_numpy(task["rows"].astype(np.int64))
    z, tgt = h[r], torch.from_numpy(task["target"].astype(np.int64))[r]
    ref = (-torch.log(torch.exp(z[torch.arange(len(r)), tgt]) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r)   # the loss kernel's form
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"loss {got_loss!r} vs float64 {loss_ref!r}, margin {margin:.3e}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for name in NAMES:
        for l, (got, p) in enumerate(zip(getattr(net, "d" + name), P[name])):
            got, want = host(got), p.grad.numpy()
            err, scale = np.abs(got - want).max(), np.abs(want).max()
            print(f"d{name}{l}: err {err:.3e}, scale {scale:.3e}")
            assert scale > 0 and err <= 2e-5 * max(scale, 1e-3), f"d{name}{l}: {err:.3e} vs scale {scale:.3e}"


def test_training_goes_down_and_repeats_bit_for_bit(env, task):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    runs = []
    for _ in range(2):
        net = make_net(env, task["g"])
        losses = [float(host(net.train_step(X, t, rows, lr=0.05))[0]) for _ in range(20)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.params()]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(p, q) for p, q in zip(runs[0][1], runs[1][1]))


def test_graph_classifier_and_on_batch_vs_float64(env, task):
    torch, ops = env["torch"], env["ops"]
    other = make_task(env, (15, 30), 90)
    clf = ops.GraphClassifier(make_net(env, task["g"]), task["g"], 3, pool="mean", seed=7)
    P = params64(torch, clf.net)
    Wc, bc = (torch.tensor(host(p).astype(np.float64)) for p in (clf.W_c, clf.b_c))
    for t, model in ((task, clf), (other, clf.on_batch(other["g"]))):
        logits = host(model.forward(dev(env, t["X"])))
        h, margin = model64(torch, t, P)
        assert margin > 1e-5, margin
        Z = torch.stack([h[a:b].sum(0) / (b - a) for a, b in zip(t["ptr"][:-1], t["ptr"][1:])])
        ref = (Z @ Wc.T + bc).detach().numpy()
        assert logits.shape == ref.shape and (np.abs(logits - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()
    with pytest.raises(env["capi"].GnnxError, match="edge attributes"):      # a batch without attributes cannot carry the stack
        clf.on_batch(ops.GraphBatch.from_coo_batched(other["g"].colidx, other["g"].colidx, other["g"].graph_ptr))
