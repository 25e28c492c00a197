"""GPU tests of semi-supervised (masked) training (run with -m gpu on an MI355X): mask -> row list, CSR restriction, the loss over a
row list, argmax / accuracy, and the pruned last layer of ops.GcnStack.

Bars (the project's own, tests/test_gpu_parity.py module docstring and its cross-entropy tests; none is new):
  * index work (row lists, restricted CSR): array_equal against numpy;
  * loss: |loss - ref| <= 1e-5 * max(1, |ref|); dlogits: |d - p / n_l| <= 1e-5 / n_l * 10 against float64; column sums within
    1e-5 * max(sum |p|);
  * pruning: BIT equality (torch.equal) between the step on the full CSR and the step on the restricted CSR -- a dropped term of a
    kept accumulator is norm * 0 -- and numeric == (tests.golden_util.same) against the oracle on the FULL CSR;
  * whole step against float64: the bounds of test_two_layer_training_step_vs_float64.
These are the workload shapes; the tight bars are tests/test_gpu_loss.py (the loss) and tests/test_gpu_mask_calls.py (the index calls).
"""
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests.golden_util import same
from tests.helpers import ROOT, synth

pytestmark = pytest.mark.gpu


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


def random_mask(seed, n, density, force=()):
    """uint8 [n]: exactly round(density * n) ones at seeded positions (at least the forced ones)."""
    m = np.zeros(n, dtype=np.uint8)
    k = int(round(density * n))
    if k:
        m[np.random.default_rng(seed).permutation(n)[:k]] = 1
    m[np.asarray(force, dtype=np.int64)] = 1
    return m


# ------------------------------------------------------------------ 1. mask -> rows
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100_003])
@pytest.mark.parametrize("density", [0.0, 0.01, 0.5, 1.0])
def test_rows_from_mask_equals_nonzero(env, n, density):
    ops, torch = env["ops"], env["torch"]
    m = random_mask(11 + n, n, density)
    rows = ops.rows_from_mask(dev(env, m))
    assert rows.dtype == torch.int32
    assert np.array_equal(host(rows), np.nonzero(m)[0].astype(np.int32))
    rows_b = ops.rows_from_mask(dev(env, m.astype(bool)))   # a bool tensor is the same mask
    assert torch.equal(rows, rows_b)


# ------------------------------------------------------------------ 2. CSR restriction
def numpy_restrict(rp, ci, vals, row_keep, col_keep):
    n = len(rp) - 1
    row_of = np.repeat(np.arange(n), np.diff(rp))
    keep = np.ones(len(ci), dtype=bool)
    if row_keep is not None:
        keep &= row_keep[row_of].astype(bool)
    if col_keep is not None:
        keep &= col_keep[ci].astype(bool)
    rp2 = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp2, row_of[keep] + 1, 1)
    return np.cumsum(rp2).astype(np.int32), ci[keep], None if vals is None else vals[keep]


@pytest.mark.parametrize("relabel", [None, "scramble"])
def test_csr_restrict_equals_numpy_filter(env, relabel):
    """R-MAT graph whose hub rows are far above 64 entries (they span many 64-entry chunks, and chunks span many short rows); on
    the relabelled graph the rows are NOT sorted by stored column id, so "stored order is kept" is visible in colidx."""
    ops, torch = env["ops"], env["torch"]
    n, e = 20_000, 400_000
    src, dst = synth.rmat_edges(21, n, e)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n, relabel=relabel)
    rp, ci = host(g.rowptr), host(g.colidx)
    assert np.diff(rp).max() > 640
    vals = synth.uniform_pm1(22, (len(ci),))
    mr, mc = random_mask(23, n, 0.3, force=np.argsort(-np.diff(rp))[:8]), random_mask(24, n, 0.5)
    for row_keep, col_keep in ((mr, None), (None, mc), (mr, mc), (None, None)):
        for with_vals in (True, False):
            rp2, ci2, v2 = ops.csr_restrict(g.rowptr, g.colidx, vals=dev(env, vals) if with_vals else None,
                                            row_keep=None if row_keep is None else dev(env, row_keep),
                                            col_keep=None if col_keep is None else dev(env, col_keep))
            erp, eci, ev = numpy_restrict(rp, ci, vals if with_vals else None, row_keep, col_keep)
            assert np.array_equal(host(rp2), erp)
            assert np.array_equal(host(ci2), eci)
            assert (v2 is None) == (not with_vals)
            if with_vals:
                assert np.array_equal(host(v2), ev)
    # everything dropped: empty rows, no entries
    rp0, ci0, _ = ops.csr_restrict(g.rowptr, g.colidx, row_keep=dev(env, np.zeros(n, dtype=np.uint8)))
    assert int(ci0.numel()) == 0 and not bool(rp0.any())
    # a mask of the wrong size never reaches the device
    with pytest.raises(ValueError):
        ops.csr_restrict(g.rowptr, g.colidx, row_keep=dev(env, np.ones(n - 1, dtype=np.uint8)))


# ------------------------------------------------------------------ 3. loss over a row list
@pytest.mark.parametrize("n,c", [(20001, 256), (777, 48), (5000, 1000), (3001, 1028), (100, 7), (9, 4), (301, 300), (301, 600)])
def test_softmax_ce_rows_shapes_masks_and_column_sums(env, n, c):
    ops, torch, capi = env["ops"], env["torch"], env["capi"]
    X = synth.uniform_pm1(900 + c, (n, c)) * 3.0
    t_all = ((7 * np.arange(n) + 3) % c).astype(np.int32)
    x = X.astype(np.float64)
    P = np.exp(x) / np.exp(x).sum(1, keepdims=True)
    for density in (0.01, 0.5):
        m = random_mask(31 + n, n, density, force=[n - 1])
        rows_np = np.nonzero(m)[0]
        nl = len(rows_np)
        t = np.where(m != 0, t_all, -1).astype(np.int32)          # unlabelled vertices carry -1
        loss_ref = oracle.cross_entropy(X[rows_np], t[rows_np])
        p = P[rows_np].copy()
        p[np.arange(nl), t[rows_np]] -= 1.0
        p /= nl
        rows = ops.rows_from_mask(dev(env, m))
        for pad in (0, 4):
            Xd = torch.zeros((n, c + pad), dtype=torch.float32, device="cuda")
            Xd[:, :c] = dev(env, X)
            Gd = torch.full((n, c + pad), 7.5, dtype=torch.float32, device="cuda")     # sentinel
            db = torch.full((c,), 7.0, dtype=torch.float32, device="cuda")
            loss, d = ops.softmax_ce_rows(Xd[:, :c], dev(env, t), rows, colsum_out=db, grad_out=Gd[:, :c])
            lv = float(host(loss)[0])
            print(f"n={n} c={c} density={density} pad={pad}: loss {lv:.8g} ref {loss_ref:.8g}")
            assert abs(lv - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
            dh = host(Gd)
            assert np.abs(dh[rows_np, :c] - p).max() <= 1e-5 / nl * 10
            others = np.ones(n, dtype=bool)
            others[rows_np] = False
            assert np.all(dh[others] == 7.5) and np.all(dh[:, c:] == 7.5)      # nothing but the listed rows is written
            scale = max(np.abs(p).sum(0).max(), 1e-12)
            assert np.abs(host(db) - p.sum(0)).max() <= 1e-5 * scale
            Gz = torch.zeros_like(Gd)
            Gz[:, :c][rows.long()] = Gd[:, :c][rows.long()]
            assert np.abs(host(db) - host(ops.colsum(Gz[:, :c]))).max() <= 1e-5 * scale
            # two runs: equal bits
            Gd2 = torch.full_like(Gd, 7.5)
            db2 = torch.empty_like(db)
            loss2, _ = ops.softmax_ce_rows(Xd[:, :c], dev(env, t), rows, colsum_out=db2, grad_out=Gd2[:, :c])
            assert torch.equal(loss, loss2) and torch.equal(Gd, Gd2) and torch.equal(db, db2)
            # two halves of the list with n_total = n_l sum to the whole
            if nl >= 2:
                la, _ = ops.softmax_ce_rows(Xd[:, :c], dev(env, t), rows[: nl // 2].contiguous(), n_total=nl, want_grad=False)
                lb, _ = ops.softmax_ce_rows(Xd[:, :c], dev(env, t), rows[nl // 2:].contiguous(), n_total=nl, want_grad=False)
                assert abs(float(host(la)[0]) + float(host(lb)[0]) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
        # a bad target INSIDE the mask is an error; outside it is never read
        tb = t.copy()
        tb[rows_np[0]] = c
        with pytest.raises(capi.GnnxError) as ei:
            ops.softmax_ce_rows(dev(env, X), dev(env, tb), rows)
        assert ei.value.status == -3
    # every row listed: the bits of ops.softmax_ce (gradient, column sums and loss), the loss within the bound
    all_rows = torch.arange(n, dtype=torch.int32, device="cuda")
    for pad in (0, 4):
        Xd = torch.zeros((n, c + pad), dtype=torch.float32, device="cuda")
        Xd[:, :c] = dev(env, X)
        db_f = torch.full((c,), 7.0, dtype=torch.float32, device="cuda")
        db_r = torch.full((c,), -7.0, dtype=torch.float32, device="cuda")
        loss_f, d_f = ops.softmax_ce(Xd[:, :c], dev(env, t_all), colsum_out=db_f)
        loss_r, d_r = ops.softmax_ce_rows(Xd[:, :c], dev(env, t_all), all_rows, colsum_out=db_r)
        assert torch.equal(d_f, d_r) and torch.equal(loss_f, loss_r) and torch.equal(db_f, db_r)
        ref = oracle.cross_entropy(X, t_all)
        assert abs(float(host(loss_r)[0]) - ref) <= 1e-5 * max(1.0, abs(ref))
    with pytest.raises(capi.GnnxError) as ei:   # an empty list: an error, never a NaN loss
        ops.softmax_ce_rows(dev(env, X), dev(env, t_all), all_rows[:0])
    assert ei.value.status == -1


# ------------------------------------------------------------------ 4. argmax / accuracy
@pytest.mark.parametrize("n,c", [(5000, 7), (3001, 47), (1000, 256), (300, 1000), (64, 1)])
def test_argmax_and_accuracy_first_maximum(env, n, c):
    ops, torch = env["ops"], env["torch"]
    X = np.round(synth.uniform_pm1(41 + c, (n, c)) * 2.0) / 4.0       # quantised to 1/4 within [-0.5, 0.5]: the maximum is tied in
    ties = (X == X.max(1, keepdims=True)).sum(1) > 1                   # most rows (in half of them at 7 classes)
    assert ties.mean() > (0.5 if c >= 16 else 0.4 if c > 1 else -1.0)
    ref = np.argmax(X, axis=1).astype(np.int32)                        # numpy: the first maximum
    for pad in (0, 3):
        Xd = torch.zeros((n, c + pad), dtype=torch.float32, device="cuda")
        Xd[:, :c] = dev(env, X)
        assert np.array_equal(host(ops.argmax_rows(Xd[:, :c])), ref)
        t = ref.copy()
        wrong = np.arange(n) % 3 == 0
        t[wrong] = (t[wrong] + 1) % max(c, 2)                          # (c == 1: class 1 does not exist, never matches)
        correct, count = ops.accuracy(Xd[:, :c], dev(env, t))
        assert (correct, count) == (int((t == ref).sum()), n)
        m = random_mask(43, n, 0.3)
        rows_np = np.nonzero(m)[0]
        tm = np.where(m != 0, t, -1).astype(np.int32)
        correct, count = ops.accuracy(Xd[:, :c], dev(env, tm), ops.rows_from_mask(dev(env, m)))
        assert (correct, count) == (int((t[rows_np] == ref[rows_np]).sum()), len(rows_np))


# ------------------------------------------------------------------ 5. + 6. the pruning identity
def masked_step(env, net, lab, X, t, pruned):
    """forward -> softmax_ce_rows -> backward (with the input gradient); everything the step produces, cloned."""
    ops, torch = env["ops"], env["torch"]
    L = lab if pruned else None
    logits = net.forward(X, labelled=L).clone()
    G = net.grad_buffer()          # the stack's own buffer (on the gather pitch when the graph asks for it)
    G.zero_()
    loss, d = ops.softmax_ce_rows(logits, t, lab.rows, colsum_out=net.db[-1], grad_out=G)
    dH = ops.aggregate_bwd(net.g, d, labelled=L).clone()
    Gin = net.backward(d, have_last_bias_grad=True, labelled=L)
    return dict(logits=logits, loss=loss.clone(), d=d.clone(), dH=dH, Gin=Gin.clone(), dW=[w.clone() for w in net.dW],
                db=[b.clone() for b in net.db])


PRUNE_CASES = [
    # (name, kind, n, e, dims, chunk, density, pad_streamed)
    ("uniform", "uniform", 3000, 24000, [32, 16, 7], 0, 0.1, None),
    ("uniform-planned", "uniform", 3000, 24000, [32, 16, 7], 8, 0.5, None),
    ("uniform-pad-streamed", "uniform", 3000, 24000, [100, 100, 47], 0, 0.1, True),
    ("rmat-half", "rmat", 1 << 17, 1_500_000, [64, 64, 47], 64, 0.5, None),
    ("rmat-1pct", "rmat", 1 << 17, 1_500_000, [64, 64, 47], 64, 0.01, None),
]


@pytest.mark.parametrize("relabel", [None, "scramble"])
@pytest.mark.parametrize("case", PRUNE_CASES, ids=[c[0] for c in PRUNE_CASES])
def test_pruned_last_layer_has_the_bits_of_the_full_step(env, case, relabel):
    ops, torch = env["ops"], env["torch"]
    _, kind, n, e, dims, chunk, density, pad = case
    src, dst = (synth.rmat_edges if kind == "rmat" else synth.uniform_edges)(51, n, e)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n, relabel=relabel)
    if chunk:
        g.make_plans(chunk, max(dims))
    deg_v = host(g.to_vertex_order(g.rowptr[1:] - g.rowptr[:-1]))
    hubs = np.argsort(-deg_v, kind="stable")[:64]
    mask = random_mask(52, n, density, force=hubs if kind == "rmat" else ())      # vertex order
    lab = g.labelled(dev(env, mask))
    nid = np.arange(n) if g.nid is None else host(g.nid).astype(np.int64)
    assert np.array_equal(host(lab.rows), np.sort(nid[np.nonzero(mask)[0]]).astype(np.int32))
    assert lab.n_labelled == int(mask.sum())
    assert int(lab.colidx.numel()) == int(lab.colidx_t.numel()) == int(lab.norm_per_nz_t.numel()) < g.nnz   # the same edge set
    if kind == "rmat":   # rows on the hub kernels before AND after the restriction
        assert g.plan.n_split_rows > 0 and g.plan_t.n_split_rows > 0
        assert lab.plan.n_split_rows > 0 and lab.plan_t.n_split_rows > 0
    net = ops.GcnStack(g, dims, seed=610, pad_streamed=pad)
    assert pad is None or net.padded
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(620 + l, (dims[l + 1],), scale=0.2)))
    X = g.to_new_order(dev(env, synth.uniform_pm1(601, (n, dims[0]))))
    # finite inputs: the loss has no max-subtraction (like the reference), and a hub row of several thousand entries sums its
    # neighbours twice over two layers -- the last weight matrix is scaled so that the largest logit is about 8
    top = float(net.forward(X).abs().max())
    assert np.isfinite(top)
    if top > 8.0:
        net.W[-1].mul_(8.0 / top)
    t_v = np.where(mask != 0, (7 * np.arange(n) + 3) % dims[-1], -1).astype(np.int32)
    t = g.to_new_order(dev(env, t_v))
    a = masked_step(env, net, lab, X, t, pruned=False)
    b = masked_step(env, net, lab, X, t, pruned=True)
    rows = lab.rows.long()
    assert torch.equal(a["logits"][rows], b["logits"][rows])
    others = torch.ones(n, dtype=torch.bool, device="cuda")
    others[rows] = False
    assert torch.equal(b["logits"][others], net.b[-1].expand(int(others.sum()), -1))     # not computed: the bias
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["d"], b["d"])
    assert torch.isfinite(a["loss"]).all()
    assert torch.equal(a["dH"], b["dH"])
    assert torch.equal(a["Gin"], b["Gin"])
    for l in range(len(dims) - 1):
        assert torch.equal(a["dW"][l], b["dW"][l]), f"dW{l}"
        assert torch.equal(a["db"][l], b["db"][l]), f"db{l}"


@pytest.mark.parametrize("relabel", [None, "scramble"])
@pytest.mark.parametrize("kind,n,e,F,chunk,density", [("uniform", 3000, 24000, 7, 0, 0.1), ("rmat", 20_000, 400_000, 47, 64, 0.01),
                                                        ("rmat", 20_000, 400_000, 47, 64, 0.5)])
def test_pruned_aggregations_equal_the_oracle_on_the_full_csr(env, kind, n, e, F, chunk, density, relabel):
    ops, torch = env["ops"], env["torch"]
    src, dst = (synth.rmat_edges if kind == "rmat" else synth.uniform_edges)(61, n, e)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n, relabel=relabel)
    if chunk:
        g.make_plans(chunk, F)
    rp, ci = oracle.coo_to_csr(src, dst, n)
    rpT, ciT = oracle.csr_transpose(rp, ci, n)
    norm = host(g.to_vertex_order(g.norm))                                  # vertex order
    hubs = np.argsort(-np.diff(rp), kind="stable")[:8]
    mask = random_mask(62, n, density, force=hubs if kind == "rmat" else ())
    rows_v = np.nonzero(mask)[0]
    lab = g.labelled(dev(env, mask))
    H = synth.uniform_pm1(63, (n, F))
    bias = synth.uniform_pm1(64, (F,), scale=0.5)
    out = ops.aggregate_fwd(g, g.to_new_order(dev(env, H)), dev(env, bias), labelled=lab)
    ref = oracle.aggregate_fwd(rp, ci, H, norm, bias)
    assert same(host(g.to_vertex_order(out))[rows_v], ref[rows_v])
    G = np.zeros((n, F), dtype=np.float32)
    G[rows_v] = synth.uniform_pm1(65, (len(rows_v), F))                     # the zero-filled gradient
    dH = ops.aggregate_bwd(g, g.to_new_order(dev(env, G)), labelled=lab)
    assert same(host(g.to_vertex_order(dH)), oracle.aggregate_bwd(rpT, ciT, G, norm))


# ------------------------------------------------------------------ 7. the whole masked step
def test_masked_training_step_vs_float64_then_training(env):
    """test_two_layer_training_step_vs_float64 with a 10 % train mask (same graph, network and bounds); then train_step for a few
    iterations -- the loss goes down -- and evaluate on a validation mask."""
    ops, torch = env["ops"], env["torch"]
    n, e, dims = 3000, 24000, [32, 16, 7]
    src, dst = synth.uniform_edges(77, n, e)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n)
    rp, ci = oracle.coo_to_csr(src, dst, n)
    _, norm = oracle.degree_norm(rp, ci, n)
    X = synth.uniform_pm1(601, (n, dims[0]))
    mask = random_mask(78, n, 0.1)
    vmask = random_mask(79, n, 0.2) & (1 - mask)
    rows_np = np.nonzero(mask)[0]
    nl = len(rows_np)
    t_all = ((7 * np.arange(n) + 3) % dims[-1]).astype(np.int32)
    t = np.where((mask | vmask) != 0, t_all, -1).astype(np.int32)
    net = ops.GcnStack(g, dims, seed=610)
    for l in range(2):
        net.b[l].copy_(dev(env, synth.uniform_pm1(620 + l, (dims[l + 1],), scale=0.2)))
    W = [host(w).astype(np.float64) for w in net.W]
    b = [host(v).astype(np.float64) for v in net.b]
    lab = g.labelled(dev(env, mask))
    Xd, td = dev(env, X), dev(env, t)
    logits = net.forward(Xd, labelled=lab)
    loss, dlog = ops.softmax_ce_rows(logits, td, lab.rows, colsum_out=net.db[-1], grad_out=net.masked_grad_buffer(lab))
    net.backward(dlog, have_last_bias_grad=True, labelled=lab)
    # ---- float64 reference
    import scipy.sparse as sp
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    S = sp.diags(norm.astype(np.float64)) @ A
    x0 = X.astype(np.float64)
    z1 = S @ (x0 @ W[0].T) + b[0]
    y1 = np.maximum(z1, 0)
    z2 = S @ (y1 @ W[1].T) + b[1]
    ex = np.exp(z2[rows_np])
    p = ex / ex.sum(1, keepdims=True)
    loss_ref = float(-np.log(p[np.arange(nl), t[rows_np]]).mean())
    dz2 = np.zeros_like(z2)
    p[np.arange(nl), t[rows_np]] -= 1
    dz2[rows_np] = p / nl
    dh2 = S.T @ dz2
    dW1, db1 = dh2.T @ y1, dz2.sum(0)
    dz1 = (dh2 @ W[1]) * (z1 > 0)
    dh1 = S.T @ dz1
    dW0, db0 = dh1.T @ x0, dz1.sum(0)
    print(f"loss {float(host(loss)[0]):.8g} ref {loss_ref:.8g}")
    assert abs(float(host(loss)[0]) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for got, ref, nm in ((net.dW[1], dW1, "dW1"), (net.db[1], db1, "db1"), (net.dW[0], dW0, "dW0"), (net.db[0], db0, "db0")):
        err = np.abs(host(got) - ref).max()
        print(f"{nm}: err {err:.3e} scale {np.abs(ref).max():.3e}")
        assert err <= 2e-5 * max(np.abs(ref).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(ref).max():.3e}"
    # ---- train_step: the loss decreases; evaluate counts the validation rows
    vrows = g.rows_of(dev(env, vmask))
    losses = [float(host(net.train_step(Xd, td, lab, lr=0.05))[0]) for _ in range(20)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    vloss, correct, count = net.evaluate(Xd, td, vrows)
    assert count == int(vrows.numel()) == int(vmask.sum()) and 0 <= correct <= count
    assert np.isfinite(float(host(vloss)[0]))
    full = net.forward(Xd)
    assert correct == int((host(full).argmax(1)[np.nonzero(vmask)[0]] == t_all[np.nonzero(vmask)[0]]).sum())
    # a second labelled set: the gradient buffer is zeroed again (rows of the first set must not linger)
    lab2 = g.labelled(dev(env, vmask))
    net.train_step(Xd, td, lab2, lr=0.05)
    Gb = net.grad_buffer()
    outside = torch.ones(n, dtype=torch.bool, device="cuda")
    outside[lab2.rows.long()] = False
    assert not bool(Gb[outside].any()) and bool(Gb[lab2.rows.long()].any())
    # the same masked step on the full CSR (the comparison leg of scripts/bench_masked_step.py) moves the parameters to the same bits
    keep = [w.clone() for w in net.W + net.b]
    net2 = ops.GcnStack(g, dims, seed=610)
    for dst_, src_ in zip(net2.W + net2.b, keep):
        dst_.copy_(src_)
    la = net.train_step(Xd, td, lab, lr=0.05)
    lb, dlog2 = ops.softmax_ce_rows(net2.forward(Xd), td, lab.rows, colsum_out=net2.db[-1], grad_out=net2.masked_grad_buffer(lab))
    net2.backward(dlog2, input_grad=False, have_last_bias_grad=True)
    net2.step(0.05)
    assert torch.equal(la, lb)
    for pa, pb in zip(net.W + net.b, net2.W + net2.b):
        assert torch.equal(pa, pb)


# ------------------------------------------------------------------ 8. the C++ mirror
@pytest.mark.parametrize("n,c", [(777, 48), (100, 7)])
def test_cpp_mirror_masked_loss_backward_and_accuracy_equal_the_python_path(env, n, c):
    ops, torch = env["ops"], env["torch"]
    exe = os.path.join(ROOT, "tests", "cpp", "test_host_masked_gpu")
    X = np.round(synth.uniform_pm1(81 + c, (n, c)) * 3.0 * 8.0) / 8.0
    mask = random_mask(82, n, 0.3)
    t = np.where(mask != 0, (7 * np.arange(n) + 3) % c, -1).astype(np.int32)
    t[np.nonzero(mask)[0][::2]] = np.argmax(X, 1)[np.nonzero(mask)[0][::2]]        # half of the masked rows are predicted right
    with tempfile.TemporaryDirectory() as td:
        cpath = os.path.join(td, "case.bin")
        with open(cpath, "wb") as f:
            np.array([n, c], dtype=np.int32).tofile(f)
            np.ascontiguousarray(X, dtype=np.float32).tofile(f)
            t.tofile(f)
            mask.astype(np.uint8).tofile(f)
        r = subprocess.run([exe, cpath, td], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "masked host api (gpu) ok" in r.stdout, r.stdout + r.stderr
        loss_c = np.fromfile(os.path.join(td, "loss.bin"), dtype=np.float32)
        grad_c = np.fromfile(os.path.join(td, "grad.bin"), dtype=np.float32).reshape(n, c)
        counts = np.fromfile(os.path.join(td, "correct.bin"), dtype=np.int64)
    rows = ops.rows_from_mask(dev(env, mask))
    loss, d = ops.softmax_ce_rows(dev(env, X), dev(env, t), rows)
    correct, count = ops.accuracy(dev(env, X), dev(env, t), rows)
    assert np.array_equal(loss_c, host(loss))
    assert np.array_equal(grad_c, host(d))                       # zero rows outside the mask included
    assert counts.tolist() == [correct, count] and 0 < correct < count
