"""GPU tests of negative sampling and link ranking (run with -m gpu on an MI355X): gnnx_csr_sample_negatives through
ops.sample_negatives / CsrGraph.sample_negatives, gnnx_rank_counts_f32 through ops.rank_counts, and what is built on them --
ops.link_metrics, EdgeSet.from_graph, GcnStack.link_evaluate.  Both kernels are integer work with one right answer: every output is
compared with tests/negative_ref.py (sets, Python integers, loops) by torch.equal.  The metrics are rationals of those integers: the
(numerator, denominator) pairs and the floats made of them are compared for equality, the float64 MRR within 1e-12 (a mean of at most
a few thousand terms in [0, 1], each correctly rounded: the sum's error is below 1e-13).

Lane mapping (gnnx_negative.hip): a wavefront owns RUN = GNNX_NEG_RUN consecutive positives; the run's (positive, draw) items go to the
64 lanes draw-fastest, 64 items per pass.  The seams are therefore the positives RUN * k (a new wavefront, with a row search of its own)
and, inside a run, the items 64 * k (a positive whose draws straddle two passes when m does not divide 64)."""
import importlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import negative_ref as nr
from tests import sddmm_ref as sr
from tests.helpers import ROOT, synth
from tests.test_negative_cpu import UNIFORM, golden_csr

pytestmark = pytest.mark.gpu

RUN = int(re.search(r"#define GNNX_NEG_RUN (\d+)", open(os.path.join(ROOT, "include", "gnnx.h")).read()).group(1))


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


def csr_of_rows(rows):
    """(rowptr, colidx) int32 of a list of ascending column lists."""
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return rowptr, colidx


def rowptr_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def assert_is_reference(env, rowptr_pos, ex, n_cols, m, seed, exclude_self, what):
    """The device draws equal the reference's, bit for bit, with the unfilled count; returns (device tensor, reference array)."""
    torch, ops = env["torch"], env["ops"]
    rowptr_ex, colidx_ex = ex
    got, unfilled = ops.sample_negatives(dev(env, rowptr_pos), m, seed, excluded=(dev(env, rowptr_ex), dev(env, colidx_ex)), n_cols=n_cols,
                                         exclude_self=exclude_self)
    ref, ref_unfilled = nr.negatives_ref(rowptr_pos, rowptr_ex, colidx_ex, n_cols, m, seed, 1 if exclude_self else 0)
    assert got.dtype == torch.int32 and tuple(got.shape) == ref.shape, what
    assert torch.equal(got.cpu(), torch.from_numpy(ref)), f"{what}: the draws differ from the reference"
    assert unfilled == ref_unfilled == int((ref < 0).sum()), what
    return got, ref


def assert_properties(rowptr_pos, ex, n_cols, neg, exclude_self):
    """No draw is stored in its row of the excluded pattern, none is the row itself under the flag, every one is inside [0, n_cols);
    -1 only where the row has nothing to draw."""
    rowptr_ex, colidx_ex = ex
    for i in range(len(rowptr_pos) - 1):
        d = neg[rowptr_pos[i]:rowptr_pos[i + 1]].reshape(-1)
        if not len(d):
            continue
        S = set(colidx_ex[rowptr_ex[i]:rowptr_ex[i + 1]].tolist())
        E = S | {i} if exclude_self and i < n_cols else S
        if len(E) == n_cols:
            assert (d == -1).all()
            continue
        assert (d >= 0).all() and (d < n_cols).all()
        assert not (set(d.tolist()) & E), f"row {i} drew an excluded column"


# ---- the sampler: crafted rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_self", [True, False])
def test_row_cases(env, exclude_self):
    """Rows of d = 0, 1, n - 2, n - 1 and n stored columns, each with and without a stored self loop; 3 positives per row, m = 3.  A
    complete row -- stored, or completed by the self column -- gives -1 and counts m per positive."""
    n = 12
    allc = list(range(n))
    rows = [[],                                     # 0: d = 0
            [5],                                    # 1: d = 1, no self loop
            [2],                                    # 2: d = 1, the self loop alone
            [c for c in allc if c not in (3, 7)],   # 3: d = n - 2 without self: one candidate under the flag
            [c for c in allc if c not in (0, 9)],   # 4: d = n - 2 with self: two candidates
            [c for c in allc if c != 5],            # 5: d = n - 1 without self: complete once the self column joins
            [c for c in allc if c != 11],           # 6: d = n - 1 with self: one candidate
            allc,                                   # 7: d = n
            [c for c in allc if c != 0],            # 8: d = n - 1 with self, the candidate is column 0
            [c for c in allc if c != 9],            # 9: d = n - 1 without self, a hole in the middle
            [0, 11],                                # 10: first and last column
            [c for c in allc if c != 11]]           # 11: d = n - 1 without self, the self column is the last column
    ex = csr_of_rows(rows)
    rowptr_pos = rowptr_of([3] * n)
    _, ref = assert_is_reference(env, rowptr_pos, ex, n, 3, 11, exclude_self, f"exclude_self = {exclude_self}")
    complete = [7] + ([5, 9, 11] if exclude_self else [])
    for i in range(n):
        assert (ref[3 * i:3 * i + 3] == -1).all() == (i in complete)
    assert int((ref < 0).sum()) == 3 * 3 * len(complete)
    assert_properties(rowptr_pos, ex, n, ref, exclude_self)


@pytest.mark.parametrize("n_rows,n_cols", [(10, 6), (6, 10)])
def test_rectangular_excluded_pattern(env, n_rows, n_cols):
    """Rows i >= n_cols have no self column to exclude; with more columns than rows the columns >= n_rows are ordinary candidates."""
    rng = np.random.default_rng(n_rows)
    rows = [sorted(rng.permutation(n_cols)[:rng.integers(0, n_cols + 1)].tolist()) for _ in range(n_rows)]
    rows[n_rows - 1] = list(range(n_cols))              # a complete row
    rows[1] = [c for c in range(n_cols) if c != 1]      # complete under the flag only
    ex = csr_of_rows(rows)
    rowptr_pos = rowptr_of(rng.integers(0, 5, size=n_rows))
    for exclude_self in (True, False):
        _, ref = assert_is_reference(env, rowptr_pos, ex, n_cols, 5, 3, exclude_self, f"{n_rows} x {n_cols}, self {exclude_self}")
        assert_properties(rowptr_pos, ex, n_cols, ref, exclude_self)


@pytest.fixture(scope="module")
def small():
    n, rowptr, colidx = golden_csr("rmat64.npz")
    return n, rowptr.astype(np.int32), colidx.astype(np.int32)


@pytest.mark.parametrize("m", [1, 3, 5, 64])
def test_every_m(env, small, m):
    n, rowptr, colidx = small
    for exclude_self in (True, False):
        assert_is_reference(env, rowptr, (rowptr, colidx), n, m, 5 + m, exclude_self, f"m = {m}, self {exclude_self}")


def test_positives_other_than_the_excluded_pattern(env, small):
    """Every second edge as positives: only their row structure counts, the whole graph stays excluded."""
    n, rowptr, colidx = small
    rows = sr.row_of_entries(rowptr)[::2]
    rowptr_pos = rowptr_of(np.bincount(rows, minlength=n))
    assert rowptr_pos[-1] == (len(colidx) + 1) // 2
    _, ref = assert_is_reference(env, rowptr_pos, (rowptr, colidx), n, 3, 8, True, "every second edge")
    assert_properties(rowptr_pos, (rowptr, colidx), n, ref, True)


def test_empty_patterns(env, small):
    torch, ops = env["torch"], env["ops"]
    n, rowptr, colidx = small
    none = np.zeros(n + 1, dtype=np.int32)
    got, unfilled = ops.sample_negatives(dev(env, none), 3, 1, excluded=(dev(env, rowptr), dev(env, colidx)))
    assert tuple(got.shape) == (0, 3) and got.dtype == torch.int32 and unfilled == 0
    empty = np.zeros(0, dtype=np.int32)
    a, _ = assert_is_reference(env, rowptr, (none, empty), n, 3, 2, True, "nothing excluded but the row itself")
    b, ub = ops.sample_negatives(dev(env, rowptr), 3, 2, excluded=None)                  # the same pattern, spelt None
    assert torch.equal(a, b) and ub == 0
    assert_is_reference(env, rowptr, (none, empty), n, 3, 2, False, "nothing excluded at all")
    got, unfilled = ops.sample_negatives(dev(env, np.zeros(1, dtype=np.int32)), 2, 1, excluded=None)    # a pattern without rows
    assert tuple(got.shape) == (0, 2) and unfilled == 0


SEAM_RUNS = {
    "one positive per row": [1] * (3 * RUN + 5),
    "one row holds all": [0, 0, 3 * RUN + 5, 0],
    "rows of one run": [RUN] * 4,
    "a row change on every run seam and next to it": [RUN - 1, 1, 1, RUN - 1, 0, 0, RUN + 1, RUN - 1, 2 * RUN, 1],
    "empty rows around the seams": [0, RUN, 0, 0, 0, RUN - 1, 0, 1, 0, 1, 2 * RUN - 2, 0, 0, 1, 0],
    "the last run is one positive": [2 * RUN, 1],
}


@pytest.mark.parametrize("name", list(SEAM_RUNS))
def test_row_changes_on_the_seams(env, name):
    """Run lengths that put a row change on, before and behind every wavefront seam (positives RUN * k); with m = 3 and m = 5 a
    positive's draws also straddle the passes of 64 items inside a run (64 is no multiple of m), with m = 1 and m = 64 they do not."""
    lengths = SEAM_RUNS[name]
    n = len(lengths)
    n_cols = max(n, 9)
    rng = np.random.default_rng(len(name))
    ex = csr_of_rows([sorted(rng.permutation(n_cols)[:rng.integers(0, 6)].tolist()) for _ in range(n)])
    rowptr_pos = rowptr_of(lengths)
    ends = set(np.cumsum(lengths).tolist())
    if name.startswith("a row change"):
        assert {RUN - 1, RUN, RUN + 1, 2 * RUN, 3 * RUN + 1, 4 * RUN} <= ends
    for m in (1, 3, 5, 64):
        assert_is_reference(env, rowptr_pos, ex, n_cols, m, 21, True, f"{name}, m = {m}")


def test_hub_row_search_depth(env):
    """A row of 5000 stored columns among n = 6000: more than 12 levels of the search; its positives spread over several wavefronts.
    The stored columns leave gaps of every kind: the first columns, the last ones, single holes."""
    n = 6000
    rng = np.random.default_rng(4)
    hub = np.sort(rng.permutation(n)[:5000])
    assert int(np.ceil(np.log2(len(hub)))) > 12
    rows = [[] for _ in range(n)]
    rows[17] = hub.tolist()
    rows[18] = list(range(1000, n))            # candidates only below the first stored column
    rows[19] = list(range(0, n - 1000))        # and only above the last one
    rows[5999] = list(range(0, n - 1))         # the self column is the one hole
    ex = csr_of_rows(rows)
    lengths = np.zeros(n, dtype=np.int64)
    lengths[[17, 18, 19, 5999]] = [300, 70, 70, 3]
    lengths[rng.integers(0, n, 200)] += 1
    rowptr_pos = rowptr_of(lengths)
    for exclude_self in (True, False):
        _, ref = assert_is_reference(env, rowptr_pos, ex, n, 5, 6, exclude_self, f"hub row, self {exclude_self}")
    d = ref[rowptr_pos[17]:rowptr_pos[18]].reshape(-1)
    assert len(set(d.tolist())) > 500 and not (set(d.tolist()) & set(hub.tolist()))


# ---- the sampler: a whole graph ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def task(env):
    """tests/golden/rmat1024.npz as a CsrGraph, with the input features of a GcnStack on it."""
    ops = env["ops"]
    d = np.load(os.path.join(ROOT, "tests", "golden", "rmat1024.npz"))
    n = int(d["X"].shape[0])
    g = ops.CsrGraph.from_coo(dev(env, d["src"]), dev(env, d["dst"]), n)
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    assert np.diff(rowptr).max() > 64 and g.nnz > 6000
    return dict(g=g, n=n, rowptr=rowptr, colidx=colidx, X=d["X"].astype(np.float32))


def test_whole_graph_properties_and_repeats(env, task):
    torch, g = env["torch"], task["g"]
    ex = (task["rowptr"], task["colidx"])
    first, ref = assert_is_reference(env, task["rowptr"], ex, task["n"], 3, 2024, True, "rmat1024")
    assert_properties(task["rowptr"], ex, task["n"], ref, True)
    again, unfilled = g.sample_negatives(3, 2024)
    assert torch.equal(first, again) and unfilled == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, _ = g.sample_negatives(3, 2024)
    side.synchronize()
    assert torch.equal(first, other)
    assert not torch.equal(first, g.sample_negatives(3, 2025)[0])
    plain, _ = g.sample_negatives(3, 2024, exclude_self=False)
    also, _ = assert_is_reference(env, task["rowptr"], ex, task["n"], 3, 2024, False, "rmat1024 without the self flag")
    assert torch.equal(plain, also)


def test_uniformity_on_the_device(env):
    """The CPU case of tests/test_negative_cpu.py drawn by the kernel: the same draws, so the same band."""
    u = UNIFORM
    rows = [[] for _ in range(u["row"] + 1)]
    rows[u["row"]] = u["S"]
    lengths = [0] * u["row"] + [u["positives"]]
    got, _ = assert_is_reference(env, rowptr_of(lengths), csr_of_rows(rows), u["n_cols"], u["m"], u["seed"], True, "uniformity case")
    counts = np.bincount(host(got).reshape(-1), minlength=u["n_cols"])
    cand = nr.candidates(u["S"], u["row"], u["n_cols"], 1)
    T = u["positives"] * u["m"]
    assert counts.sum() == T and counts[cand].sum() == T
    worst = float((np.abs(counts[cand] - T / 16) / np.sqrt(T * (1 / 16) * (15 / 16))).max())
    print(f"count = 16, {T} draws on the device: largest deviation {worst:.2f} sd")
    assert worst <= 5.0


# ---- rank counts and metrics ------------------------------------------------------------------------------------------------------
SPECIAL = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], dtype=np.float32)


def special_scores(P, m, seed, skip):
    rng = np.random.default_rng(seed)
    s = SPECIAL[rng.integers(0, len(SPECIAL), P)]
    s[:len(SPECIAL)] = SPECIAL[:min(P, len(SPECIAL))]                    # every value as a positive score
    q = SPECIAL[rng.integers(0, len(SPECIAL), (P, m))]
    neg = rng.integers(0, 50, (P, m)).astype(np.int32)
    if skip:
        neg[rng.random((P, m)) < 0.2] = -1
        neg[P // 2] = -1                                                   # a positive all of whose draws are skipped
    return s, q, neg


@pytest.mark.parametrize("m", [1, 2, 5, 17, 63, 64, 65, 257])
def test_rank_counts_vs_reference(env, m):
    """Scores from {-inf, -1, -0, 0, 1, inf, NaN}: ties, the two zeros and NaN on both sides; skipped draws; every lane-group width
    (m = 1, 2, 5, 17 .. 64) and rows of more than one pass (65, 257); P = 37 is no multiple of the positives of a block."""
    torch, ops = env["torch"], env["ops"]
    P = 37
    for skip in (True, False):
        s, q, neg = special_scores(P, m, 100 + m, skip)
        got = ops.rank_counts(dev(env, s), dev(env, q), dev(env, neg) if skip else None)
        ref = nr.rank_counts_ref(s, q, neg if skip else None)
        for name, a, b in zip(("greater", "equal", "valid"), got, ref):
            assert a.dtype == torch.int32 and torch.equal(a.cpu(), torch.from_numpy(b)), f"m = {m}, skip = {skip}: {name}"
    g, e, v = ref
    assert g.sum() > 0 and e.sum() > 0 and (v < m).any()


def assert_metrics_equal(got, ref, ks):
    assert got["n_pos"] == ref["n_pos"] and got["n_valid"] == ref["n_valid"]
    for k in ks:
        assert got[f"hits@{k}"] == float(ref[f"hits@{k}"]), k
    for name in ("auc", "auc_grouped"):
        num, den = got[name + "_fraction"]
        assert den > 0 and Fraction(num, den) == ref[name], name
        assert got[name] == num / den == float(ref[name]), name
    err = abs(Fraction(got["mrr"]) - ref["mrr"])
    print(f"mrr {got['mrr']!r}, off the exact rational by {float(err):.2e}")
    assert err <= Fraction(1, 10 ** 12)


@pytest.mark.parametrize("m", [1, 5, 64])
def test_link_metrics_vs_reference(env, m):
    ops = env["ops"]
    ks = (1, 3, 10)
    s, q, neg = special_scores(211, m, 7 + m, True)
    assert_metrics_equal(ops.link_metrics(dev(env, s), dev(env, q), dev(env, neg), ks=ks), nr.metrics_ref(s, q, neg, ks), ks)
    assert_metrics_equal(ops.link_metrics(dev(env, s), dev(env, q), ks=ks), nr.metrics_ref(s, q, None, ks), ks)
    rng = np.random.default_rng(m)                       # distinct real scores: no ties
    s, q = rng.standard_normal(300).astype(np.float32) + 1, rng.standard_normal((300, m)).astype(np.float32)
    ref = nr.metrics_ref(s, q, None, ks)
    assert_metrics_equal(ops.link_metrics(dev(env, s), dev(env, q), ks=ks), ref, ks)
    assert ref["auc"] > Fraction(1, 2)


# ---- EdgeSet.from_graph and link_evaluate -----------------------------------------------------------------------------------------
DIMS = [16, 32, 16]


def make_net(env, task, seed=950):
    ops = env["ops"]
    net = ops.GcnStack(task["g"], DIMS, seed=seed)
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    return net


def test_edge_set_from_graph(env, task):
    """The pattern holds every positive with target 1; no entry with target 0 is an edge or a self pair; the negatives are the distinct
    draws of g.sample_negatives (repeats collapse), listed per row."""
    ops, g, n = env["ops"], task["g"], task["n"]
    rowptr, colidx = task["rowptr"], task["colidx"]
    edges_of = set(zip(sr.row_of_entries(rowptr).tolist(), colidx.tolist()))
    for m, positives in ((1, None), (2, "half")):
        if positives is None:
            pos_rowptr, pos_colidx = rowptr, colidx
            e = ops.EdgeSet.from_graph(g, m, 31)
        else:
            keep = np.arange(len(colidx)) % 2 == 0
            pos_rowptr = rowptr_of(np.bincount(sr.row_of_entries(rowptr)[keep], minlength=n))
            pos_colidx = colidx[keep]
            e = ops.EdgeSet.from_graph(g, m, 31, positives=(dev(env, pos_rowptr), dev(env, pos_colidx)))
        pos = set(zip(sr.row_of_entries(pos_rowptr).tolist(), pos_colidx.tolist()))
        pairs = list(zip(sr.row_of_entries(host(e.rowptr)).tolist(), host(e.colidx).tolist()))
        target = host(e.target)
        assert pairs == sorted(set(pairs)) and set(target.tolist()) == {0.0, 1.0}
        assert {p for p, t in zip(pairs, target) if t == 1.0} == pos
        negs = {p for p, t in zip(pairs, target) if t == 0.0}
        assert negs and not (negs & edges_of) and all(a != b for a, b in negs)
        ref, _ = nr.negatives_ref(pos_rowptr, rowptr, colidx, n, m, 31, 1)
        assert negs == set(zip(np.repeat(sr.row_of_entries(pos_rowptr), m).tolist(), ref.reshape(-1).tolist()))
        assert e.n == n and e.nnz == len(pos) + len(negs) <= len(pos) * (1 + m)


def test_epochs_with_fresh_negatives_repeat_bit_for_bit(env, task):
    torch, ops = env["torch"], env["ops"]
    X = dev(env, task["X"])
    runs = []
    for _ in range(2):
        net = make_net(env, task)
        losses = [float(host(net.link_train_step(X, ops.EdgeSet.from_graph(task["g"], 1, seed=epoch), lr=1e-5))[0]) for epoch in range(20)]
        assert all(np.isfinite(losses)), losses
        runs.append((losses, [p.clone() for p in net.W + net.b]))
    assert runs[0][0] == runs[1][0]
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)
    assert not torch.equal(ops.EdgeSet.from_graph(task["g"], 1, seed=0).colidx, ops.EdgeSet.from_graph(task["g"], 1, seed=1).colidx)


@pytest.mark.parametrize("m", [1, 4])
def test_link_evaluate_is_the_composition(env, task, m):
    """link_evaluate = the reference metrics of sddmm_ref scores on the positives and on their reference draws (F = 16).  One row of the
    held-out set is made complete in a copy of the graph, so that unfilled draws pass through the scoring."""
    ops, n = env["ops"], task["n"]
    rowptr, colidx = task["rowptr"], task["colidx"]
    keep = np.arange(len(colidx)) % 3 == 0                                   # the held-out edges: every third entry
    pos_rowptr = rowptr_of(np.bincount(sr.row_of_entries(rowptr)[keep], minlength=n))
    pos_colidx = colidx[keep]
    net = make_net(env, task)
    X = dev(env, task["X"])
    ks = (1, 10, 50)
    got = net.link_evaluate(X, task["g"], (dev(env, pos_rowptr), dev(env, pos_colidx)), m, 77, ks=ks)
    Z = host(net.forward(X))
    assert Z.shape == (n, 16)
    neg, unfilled = nr.negatives_ref(pos_rowptr, rowptr, colidx, n, m, 77, 1)
    assert unfilled == 0
    s = sr.sddmm_ref(pos_rowptr, pos_colidx, Z, Z)
    q = sr.sddmm_ref(pos_rowptr * m, neg.reshape(-1), Z, Z).reshape(-1, m)
    assert_metrics_equal(got, nr.metrics_ref(s, q, neg, ks), ks)
    # an EdgeSet as positives, and a graph with a complete row: its draws are -1, scored at column 0 and skipped
    full = int(np.argmax(np.diff(pos_rowptr)))
    rows2 = [colidx[rowptr[i]:rowptr[i + 1]].tolist() if i != full else list(range(n)) for i in range(n)]
    rp2, ci2 = csr_of_rows(rows2)
    g2 = ops.CsrGraph(n, dev(env, rp2), dev(env, ci2))
    got2 = net.link_evaluate(X, g2, (dev(env, pos_rowptr), dev(env, pos_colidx)), m, 77, ks=ks)
    neg2, unfilled2 = nr.negatives_ref(pos_rowptr, rp2, ci2, n, m, 77, 1)
    assert unfilled2 == m * (pos_rowptr[full + 1] - pos_rowptr[full]) > 0
    q2 = sr.sddmm_ref(pos_rowptr * m, np.maximum(neg2.reshape(-1), 0), Z, Z).reshape(-1, m)
    assert_metrics_equal(got2, nr.metrics_ref(s, q2, neg2, ks), ks)
    assert got2["n_valid"] == got["n_valid"] - unfilled2
