"""CPU checks of negative sampling and link ranking: the restatement (tests/negative_ref.py) pinned to literals worked by hand on a
5-vertex graph, the header's closed-form selection r + J(r) against the set difference for every r of every row of a golden graph, the
uniformity of the draw, the presence of the new C-ABI entries, their argument validation (which needs no device) and the signatures of
the new Python calls.

Uniformity: T = 16 000 draws on one row with count = 16 candidates; a bucket is binomial with mean T / 16 = 1000 and standard deviation
sqrt(T * (1/16) * (15/16)) = 30.6; every bucket must lie within 5 of them (a 6e-7 event per bucket).  The seed's reference was confirmed
to stay inside the band (largest deviation 1.47 sd) before it was fixed; tests/test_gpu_negative.py reruns the case on the device."""
import ctypes as C
import importlib
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import negative_ref as nr
from tests.helpers import ROOT, synth

# the 5-vertex graph worked by hand.  Excluded rows: 0: {1, 2}; 1: {0, 1, 3} (a stored self loop); 2: {}; 3: {0 .. 4} (complete);
# 4: {0, 1, 2, 3} (complete once the self column joins).  Positives: 2, 1, 2, 1, 1 entries in rows 0 .. 4 (only the structure counts).
HAND_ROWPTR_EX = np.array([0, 2, 5, 5, 10, 14], dtype=np.int32)
HAND_COLIDX_EX = np.array([1, 2, 0, 1, 3, 0, 1, 2, 3, 4, 0, 1, 2, 3], dtype=np.int32)
HAND_ROWPTR_POS = np.array([0, 2, 3, 5, 6, 7], dtype=np.int32)
HAND_SEED, HAND_M = 2024, 2
# h of (row i, entry j, draw t) at seed 2024, from an independent evaluation of the key with synth.splitmix64
HAND_KEYS = {(0, 0, 0): 0x0A7C5F29E976084C, (0, 0, 1): 0x47A4240627CCF034, (0, 1, 0): 0x5AFFA69232AC00EA, (0, 1, 1): 0x14522B8D72B246BC,
             (1, 0, 0): 0x067D1AAC1899384B, (1, 0, 1): 0xB4625D3721A857C7, (2, 0, 0): 0x65575A405D1D74B6, (2, 0, 1): 0xE9EB986490EC7769,
             (2, 1, 0): 0x923CC13F0E1A4EA6, (2, 1, 1): 0x948491DCF3B24015, (3, 0, 0): 0x9423DB8C92D9B898, (4, 0, 1): 0x9DC034937D40808D}
# with the self flag the candidates are 0: [3, 4], 1: [2, 4], 2: [0, 1, 3, 4], 3: [], 4: []; r = floor(h * count / 2^64):
#   row 0: h / 2^64 = .04, .28 | .36, .08 -> r = 0, 0 | 0, 0 -> 3, 3 | 3, 3        row 1: .03, .70 -> r = 0, 1 -> 2, 4
#   row 2: .40, .91 | .57, .58 -> r = 1, 3 | 2, 2 -> 1, 4 | 3, 3                     rows 3, 4: nothing to draw, 2 * 2 unfilled
HAND_NEG_SELF = [[3, 3], [3, 3], [2, 4], [1, 4], [3, 3], [-1, -1], [-1, -1]]
# without it: 0: [0, 3, 4], 1: [2, 4], 2: [0, 1, 2, 3, 4], 3: [], 4: [4]
#   row 0: r = 0, 0 | 1, 0 -> 0, 0 | 3, 0      row 1: as above      row 2: r = 1, 4 | 2, 2 -> 1, 4 | 2, 2
#   row 4: r = 0 -> 4, 4; only row 3 is unfilled
HAND_NEG_PLAIN = [[0, 0], [3, 0], [2, 4], [1, 4], [2, 2], [-1, -1], [4, 4]]


def test_key_is_the_header_formula_on_synth_splitmix64():
    G = np.uint64(nr.GOLDEN)

    def sm(x):
        return synth.splitmix64(np.array([x], dtype=np.uint64))[0]

    for (i, j, t), h in HAND_KEYS.items():
        assert nr.key(HAND_SEED, i, j, t) == h, (i, j, t)
        with np.errstate(over="ignore"):
            s = sm(np.uint64(HAND_SEED) ^ np.uint64(0x6E65676174697665))
            assert int(sm(sm(s ^ (np.uint64((i << 32) | j) * G)) ^ (np.uint64(t) * G))) == h
    # all 64 bits of the seed count, and the domain constant separates the draw from the neighbour sampler's key chain
    assert nr.key(1, 3, 4, 0) != nr.key(1 + 2 ** 32, 3, 4, 0)
    from tests import sample_ref
    assert nr.fin(nr.fin(7) ^ 5) == int(sample_ref.finaliser(np.uint64(int(sample_ref.finaliser(np.uint64(7))) ^ 5)))
    assert nr.DOMAIN == int.from_bytes(b"negative", "big")


@pytest.mark.parametrize("flags,expect,unfilled", [(1, HAND_NEG_SELF, 4), (0, HAND_NEG_PLAIN, 2)])
def test_reference_equals_the_hand_worked_graph(flags, expect, unfilled):
    neg, n_unfilled = nr.negatives_ref(HAND_ROWPTR_POS, HAND_ROWPTR_EX, HAND_COLIDX_EX, 5, HAND_M, HAND_SEED, flags)
    assert neg.dtype == np.int32 and neg.tolist() == expect
    assert n_unfilled == unfilled


def test_candidates_are_the_set_difference():
    assert nr.candidates([1, 2], 0, 5, 1).tolist() == [3, 4]
    assert nr.candidates([1, 2], 0, 5, 0).tolist() == [0, 3, 4]
    assert nr.candidates([0, 1, 3], 1, 5, 1).tolist() == [2, 4]            # a stored self loop: the flag changes nothing
    assert nr.candidates([0, 1, 2, 3, 4], 3, 5, 0).tolist() == []          # a complete row
    assert nr.candidates([0, 1, 2, 3], 4, 5, 1).tolist() == [] and nr.candidates([0, 1, 2, 3], 4, 5, 0).tolist() == [4]
    assert nr.candidates([0, 2], 7, 4, 1).tolist() == [1, 3]               # i >= n_cols: there is no self column to exclude
    assert nr.draw(1, 0, 0, 0, np.zeros(0, dtype=np.int64)) == -1


def golden_csr(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name))
    n = int(d["X"].shape[0])
    pairs = np.unique(np.stack([d["src"], d["dst"]], 1).astype(np.int64), axis=0)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n))])
    return n, rowptr, pairs[:, 1]


def test_closed_form_selection_equals_the_set_difference_on_every_row():
    """r + J(r), with the self adjustment, is the r-th element of [0, n_cols) \\ E: every r of every row of the golden R-MAT graph of 64
    vertices, both flag values, square and with fewer columns than rows (rows i >= n_cols have no self column)."""
    n, rowptr, colidx = golden_csr("rmat64.npz")
    assert (np.diff(rowptr) == 0).any() and np.diff(rowptr).max() > 16
    checked = 0
    for n_cols in (n, 40):
        for i in range(n):
            S = colidx[rowptr[i]:rowptr[i + 1]]
            S = S[S < n_cols]
            for flags in (0, 1):
                cand = nr.candidates(S, i, n_cols, flags)
                assert len(cand) == n_cols - len(nr.excluded_set(S, i, n_cols, flags))
                got = [nr.select_by_formula(S, i, n_cols, flags, r) for r in range(len(cand))]
                assert got == cand.tolist(), (n_cols, i, flags)
                checked += len(cand)
    assert checked > 10_000
    # the edges of the formula: nothing stored, everything but one stored, the self column first / last / only candidate
    for S, i, n_cols in (([], 0, 4), ([], 3, 4), ([0, 1, 2], 3, 5), ([1, 2, 3], 0, 5), ([0, 1, 2, 3], 9, 5), ([0, 2, 4], 3, 5)):
        for flags in (0, 1):
            cand = nr.candidates(S, i, n_cols, flags)
            assert [nr.select_by_formula(S, i, n_cols, flags, r) for r in range(len(cand))] == cand.tolist()


UNIFORM = dict(seed=0, row=7, n_cols=20, S=[2, 9, 15], positives=4000, m=4)   # count = 20 - 3 - 1 = 16, T = 16 000


def test_draws_are_uniform_on_one_row():
    u = UNIFORM
    cand = nr.candidates(u["S"], u["row"], u["n_cols"], 1)
    T = u["positives"] * u["m"]
    assert len(cand) == 16 and T == 16_000
    counts = np.zeros(u["n_cols"], dtype=np.int64)
    for j in range(u["positives"]):
        for t in range(u["m"]):
            counts[nr.draw(u["seed"], u["row"], j, t, cand)] += 1
    assert counts.sum() == T and counts[[2, 7, 9, 15]].sum() == 0
    sd = np.sqrt(T * (1 / 16) * (15 / 16))
    worst = float((np.abs(counts[cand] - T / 16) / sd).max())
    print(f"count = 16, {T} draws: largest deviation {worst:.2f} sd")
    assert worst <= 5.0


def test_rank_counts_and_metrics_of_the_reference_by_hand():
    inf, nan = float("inf"), float("nan")
    s = [0.0, 1.0, nan, -inf, 2.0]
    q = [[-0.0, 1.0, -1.0, nan], [1.0, 1.0, 2.0, 0.0], [0.0, 1.0, 2.0, 3.0], [-inf, inf, nan, -1.0], [3.0, 3.0, 1.0, 1.0]]
    neg = [[5, 5, 5, 5], [5, 5, -1, 5], [5, 5, 5, 5], [5, 5, 5, 5], [-1, 5, 5, -1]]
    g, e, v = nr.rank_counts_ref(s, q, neg)
    assert g.tolist() == [1, 0, 0, 2, 1] and e.tolist() == [1, 2, 0, 1, 0] and v.tolist() == [3, 3, 0, 3, 2]
    g0, e0, v0 = nr.rank_counts_ref(s, q)
    assert g0.tolist() == [1, 1, 0, 2, 2] and e0.tolist() == [1, 2, 0, 1, 0] and v0.tolist() == [3, 4, 0, 3, 4]
    mt = nr.metrics_ref(s, q, neg, ks=(1, 2, 3))
    # ranks 1 + greater + equal = 3, 3, 1, 4, 2
    assert mt["mrr"] == (Fraction(1, 3) + Fraction(1, 3) + 1 + Fraction(1, 4) + Fraction(1, 2)) / 5
    assert (mt["hits@1"], mt["hits@2"], mt["hits@3"]) == (Fraction(1, 5), Fraction(2, 5), Fraction(4, 5))
    # below: 1, 1, 0, 0, 1 -> (3 + 4 / 2) / 11
    assert mt["auc_grouped"] == Fraction(2 * 3 + 4, 2 * 11) and mt["n_valid"] == 11 and mt["n_pos"] == 5
    # global: positives 0, 1, -inf, 2 against the 15 valid non-NaN negatives {-0, 1, -1 | 1, 1, 0 | 0, 1, 2, 3 | -inf, inf, -1 | 3, 1}
    #   0: below -1, -1, -inf = 3, ties -0, 0, 0 = 3;  1: below 3 + 3 = 6, ties 5;  -inf: below 0, ties 1;  2: below 11, ties 1
    assert mt["auc"] == Fraction(2 * (3 + 6 + 0 + 11) + (3 + 5 + 1 + 1), 2 * 4 * 15)
    empty = nr.metrics_ref([nan], [[1.0]], None)
    assert empty["auc"] is None and empty["auc_grouped"] is None and empty["mrr"] == 1


def test_the_two_forms_of_the_global_auc_count_agree():
    rng = np.random.default_rng(3)
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, 0.5, 2.5])
    poss, negs = rng.choice(vals, 300).tolist(), rng.choice(vals, 700).tolist()
    loop = sum(2 if a > b else 1 if a == b else 0 for a in poss for b in negs)
    assert nr.auc_wins2(poss, negs) == loop and nr.auc_wins2(poss, negs, pair_limit=0) == loop
    poss, negs = rng.standard_normal(200).tolist(), rng.standard_normal(300).tolist()
    loop = sum(2 if a > b else 1 if a == b else 0 for a in poss for b in negs)
    assert nr.auc_wins2(poss, negs) == loop and nr.auc_wins2(poss, negs, pair_limit=0) == loop


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_header_signatures_and_exports(capi):
    L = capi.lib()
    names = capi.declared_symbols()
    for name, n_args in (("gnnx_csr_sample_negatives", 15), ("gnnx_rank_counts_f32", 9)):
        assert name in names and hasattr(L, name) and len(capi._SIGS[name]) == n_args
    header = open(capi.HEADER_PATH).read()
    for word in ("GNNX_NEG_EXCLUDE_SELF 1u", "GNNX_NEG_RUN 64", "GNNX_NEG_WORKSPACE_BYTES 256", "0x6E65676174697665"):
        assert word in header, word
    assert "gnnx_negative.hip" in open(os.path.join(ROOT, "gnn.cpp_amd", "csrc", "Makefile")).read()


def test_argument_validation_without_device(capi):
    """Validation happens before any HIP call, so these return statuses even with no GPU."""
    L = capi.lib()
    INVALID, WORKSPACE = -1, -4
    p = C.c_void_p(4096)    # never dereferenced: every call below fails before a device is touched
    out = C.c_int64(-5)

    def sample(n_rows=4, n_cols=4, nnz_pos=6, rowptr_pos=p, nnz_ex=5, rowptr_ex=p, colidx_ex=p, m=2, seed=1, flags=1, neg=p, out=C.byref(out),
               ws=p, wsb=256):
        return L.gnnx_csr_sample_negatives(n_rows, n_cols, nnz_pos, rowptr_pos, nnz_ex, rowptr_ex, colidx_ex, m, seed, flags, neg, out, ws, wsb,
                                           None)

    for name in ("n_rows", "n_cols", "nnz_pos", "nnz_ex"):
        assert sample(**{name: -1}) == INVALID, name
    assert sample(m=0) == INVALID and sample(m=-2) == INVALID
    assert sample(nnz_pos=1 << 31, m=1) == INVALID
    assert sample(nnz_pos=1 << 30, m=2) == INVALID and sample(nnz_pos=3, m=(1 << 31) // 3 + 1) == INVALID
    assert sample(nnz_ex=1 << 31) == INVALID
    for name in ("rowptr_pos", "rowptr_ex", "colidx_ex", "neg", "out"):
        assert sample(**{name: None}) == INVALID, name
        assert b"null" in L.gnnx_last_error()
    assert sample(ws=None) == WORKSPACE and sample(wsb=255) == WORKSPACE
    assert out.value == -5          # a refused call writes nothing
    # valid empty results need no device either: no rows, no positives (colidx_ex and neg may then be null)
    assert sample(n_rows=0, nnz_pos=0, nnz_ex=0, colidx_ex=None, neg=None) == 0 and out.value == 0
    out.value = -5
    assert sample(nnz_pos=0, neg=None) == 0 and out.value == 0

    def rank(n_pos=3, m=2, s=p, q=p, neg=None, g=p, e=p, v=p):
        return L.gnnx_rank_counts_f32(n_pos, m, s, q, neg, g, e, v, None)

    assert rank(n_pos=-1) == INVALID and rank(n_pos=1 << 31) == INVALID
    assert rank(m=0) == INVALID and rank(m=-1) == INVALID
    for name in ("s", "q", "g", "e", "v"):
        assert rank(**{name: None}) == INVALID, name
    assert rank(n_pos=0, s=None, q=None, g=None, e=None, v=None) == 0


def test_python_signatures():
    ops = importlib.import_module("gnncpp_amd.ops")

    def params(f):
        return list(inspect.signature(f).parameters)

    def default(f, name):
        return inspect.signature(f).parameters[name].default

    assert params(ops.sample_negatives)[:6] == ["rowptr", "m", "seed", "excluded", "n_cols", "exclude_self"]
    assert default(ops.sample_negatives, "n_cols") is None and default(ops.sample_negatives, "exclude_self") is True
    assert params(ops.rank_counts) == ["pos_scores", "neg_scores", "neg"] and default(ops.rank_counts, "neg") is None
    assert params(ops.link_metrics) == ["pos_scores", "neg_scores", "neg", "ks"] and default(ops.link_metrics, "ks") == (10, 50, 100)
    assert params(ops.CsrGraph.sample_negatives)[:4] == ["self", "m", "seed", "positives"]
    assert default(ops.CsrGraph.sample_negatives, "positives") is None
    assert params(ops.EdgeSet.from_graph) == ["g", "m", "seed", "positives"] and default(ops.EdgeSet.from_graph, "positives") is None
    assert params(ops.GcnStack.link_evaluate) == ["self", "X", "g", "positives", "m", "seed", "ks"]
    assert ops.NEG_EXCLUDE_SELF == 1
    assert "collapse" in ops.EdgeSet.from_graph.__doc__ and "NaN" in ops.link_metrics.__doc__
