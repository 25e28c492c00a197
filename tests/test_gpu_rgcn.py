"""GPU tests of ops.RgcnStack (run with -m gpu on an MI355X): a 2-layer stack, dims [8, 16, 4], R = 4 relations, with a weight per
relation (n_bases None) and with 2 bases, on a batch of three graphs with n = 60 vertices and about 3 stored entries a row (duplicate
edges and self loops in the list: the last duplicate gives the entry its type).

Bars (none is new; tests/test_gpu_gine.py and tests/test_gpu_sage.py use them at the same depth): one train_step against a float64
autograd model on the CPU within 1e-5 * max(1, |ref|) for the loss and 2e-5 * max(|ref|_max, 1e-3) for every parameter gradient, C
included; the logits of GraphClassifier, and of on_batch on a batch of another size, within the first bar.  Before comparing, no ReLU
pre-activation of the float64 model may lie within 1e-5 of zero (the fixed seeds were checked on the CPU).  Twenty steps lower the loss
and repeat bit for bit."""
import numpy as np
import pytest

from tests.helpers import synth
from tests.test_gpu_sage import dev, env, host  # noqa: F401

pytestmark = pytest.mark.gpu

DIMS, R, SEED = [8, 16, 4], 4, 5200
BASES = pytest.mark.parametrize("n_bases", (None, 2))


def make_task(env, sizes, seed):
    """A GraphBatch of len(sizes) graphs with 3 n_k listed edges each and their types; the host copies the float64 model reads."""
    ops = env["ops"]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    parts = [synth.uniform_edges(seed + k, n_k, 3 * n_k) for k, n_k in enumerate(sizes)]
    src = np.concatenate([s + o for (s, _), o in zip(parts, ptr)]).astype(np.int32)
    dst = np.concatenate([d + o for (_, d), o in zip(parts, ptr)]).astype(np.int32)
    n, etype = int(ptr[-1]), np.random.default_rng(seed).integers(0, R, len(src)).astype(np.int32)
    g = ops.GraphBatch.from_coo_batched(dev(env, src), dev(env, dst), dev(env, ptr)).set_edge_type(dev(env, src), dev(env, dst), dev(env, etype), R)
    rowptr, colidx = host(g.rowptr).astype(np.int64), host(g.colidx).astype(np.int64)
    last = {(s, d): x for x, (s, d) in enumerate(zip(src, dst))}        # of duplicate edges the last
    rows_e = np.repeat(np.arange(n), np.diff(rowptr))
    types = np.array([etype[last[(r, c)]] for r, c in zip(rows_e, colidx)])
    count = np.zeros((n, R))
    np.add.at(count, (rows_e, types), 1)
    assert np.array_equal(host(g.entry_type), types) and len(colidx) < len(src) and (src == dst).any()
    assert np.array_equal(host(g.typed_norm), (1 / count[rows_e, types]).astype(np.float32))
    return dict(g=g, n=n, ptr=ptr, rows_e=rows_e, colidx=colidx, types=types, norm=1 / count[rows_e, types],
                X=synth.uniform_pm1(seed + 51, (n, DIMS[0])), target=((5 * np.arange(n) + 1) % DIMS[-1]).astype(np.int32),
                rows=np.arange(0, n, 3, dtype=np.int32))


@pytest.fixture(scope="module")
def task(env):
    return make_task(env, (20, 25, 15), 70)


def make_net(env, g, n_bases):
    net = env["ops"].RgcnStack(g, DIMS, R, n_bases=n_bases, seed=SEED)
    for l, b in enumerate(net.b):
        b.copy_(dev(env, synth.uniform_pm1(SEED + 100 + l, tuple(b.shape), scale=0.2)))
    return net, ("W_0", "V", "b") + (("C",) if n_bases else ())


def model64(torch, t, P):
    """(h [n, dims[-1]], the smallest |ReLU pre-activation|) of the float64 stack on float64 copies P of the device's parameters."""
    rows_e, cols, types = (torch.from_numpy(t[k]) for k in ("rows_e", "colidx", "types"))
    h, norm, margin, L = torch.from_numpy(t["X"].astype(np.float64)), torch.from_numpy(t["norm"]), np.inf, len(P["W_0"])
    for l in range(L):
        w = (P["C"][l] if "C" in P else torch.eye(R, dtype=torch.float64))[types] * norm[:, None]
        M = torch.zeros(t["n"], w.shape[1], h.shape[1], dtype=torch.float64).index_add(0, rows_e, w[:, :, None] * h[cols][:, None, :])
        Z = h @ P["W_0"][l].T + M.reshape(t["n"], -1) @ P["V"][l].T + P["b"][l]
        if l + 1 < L:
            margin = min(margin, float(Z.detach().abs().min()))
        h = torch.relu(Z) if l + 1 < L else Z
    return h, margin


def params64(torch, net, names):
    return {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in names}


@BASES
def test_one_step_vs_float64(env, task, n_bases):
    torch = env["torch"]
    net, names = make_net(env, task["g"], n_bases)
    P = params64(torch, net, names)
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
    for name in names:
        for l, (got, p) in enumerate(zip(getattr(net, "d" + name), P[name])):
            got, want = host(got), p.grad.numpy()
            err, scale = np.abs(got - want).max(), np.abs(want).max()
            print(f"d{name}{l}: err {err:.3e}, scale {scale:.3e}")
            assert scale > 0 and err <= 2e-5 * max(scale, 1e-3), f"d{name}{l}: {err:.3e} vs scale {scale:.3e}"


@BASES
def test_training_goes_down_and_repeats_bit_for_bit(env, task, n_bases):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    runs = []
    for _ in range(2):
        net, _ = make_net(env, task["g"], n_bases)
        losses = [float(host(net.train_step(X, t, rows, lr=0.05))[0]) for _ in range(20)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.params()]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(p, q) for p, q in zip(runs[0][1], runs[1][1]))


@BASES
def test_graph_classifier_on_batch_and_link_step(env, task, n_bases):
    torch, ops = env["torch"], env["ops"]
    other = make_task(env, (15, 30), 90)
    net, names = make_net(env, task["g"], n_bases)
    clf = ops.GraphClassifier(net, task["g"], 3, pool="mean", seed=7)
    P = params64(torch, clf.net, names)
    Wc, bc = (torch.tensor(host(p).astype(np.float64)) for p in (clf.W_c, clf.b_c))
    for t, model in ((task, clf), (other, clf.on_batch(other["g"]))):
        logits = host(model.forward(dev(env, t["X"])))
        h, margin = model64(torch, t, P)
        assert margin > 1e-5, margin
        Z = torch.stack([h[a:b].sum(0) / (b - a) for a, b in zip(t["ptr"][:-1], t["ptr"][1:])])
        ref = (Z @ Wc.T + bc).detach().numpy()
        assert logits.shape == ref.shape and (np.abs(logits - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all()
    with pytest.raises(env["capi"].GnnxError, match="relation types"):       # a batch without types cannot carry the stack
        clf.on_batch(ops.GraphBatch.from_coo_batched(other["g"].colidx, other["g"].colidx, other["g"].graph_ptr))
    loss = net.link_train_step(dev(env, task["X"]), ops.EdgeSet.from_graph(task["g"], 2, 11), lr=0.01)
    assert np.isfinite(host(loss)).all()
