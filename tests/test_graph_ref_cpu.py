"""The yardstick of tests/test_gpu_graph_build.py held to its own references, without a GPU, and the proof that the cases of
that file can fail.

  * tests/graph_ref.py's unweighted and weighted builders (the dense definition and the stable-sort form) equal the C oracle on
    seeded R-MAT lists and the compiled reference's own edge lists in tests/golden/;
  * degree_norm_ref equals oracle.degree_norm bit for bit;
  * the row-length list of the degree-block test holds every hand-over and chunk-tail length and sits where its docstring says; with
    the seeded s a sum taken in ascending order, or as 64-entry partial sums, differs in bits on at least 90 % of the long rows; the
    libm table differs from the rounded rsqrt at the 1057-entry row; the seeded weighted list has the duplicate runs that tell the
    last entry of a run from any other;
  * NaN under GNNX_CSR_DROP_TRUNCATED_ZERO: kept by the restatement ("dropped iff -1 < w < 1") and by the oracle."""
import numpy as np
import pytest

import oracle
from tests import graph_ref as gr
from tests.golden_util import load_case
from tests.helpers import synth

GRAPHS = [(3001, 60000, 901), (5000, 120000, 902)]


@pytest.fixture(scope="module", params=GRAPHS, ids=lambda p: f"rmat{p[0]}")
def edges(request):
    n, e, seed = request.param
    src, dst = synth.rmat_edges(seed, n, e)
    key = src.astype(np.int64) * n + dst
    assert len(np.unique(key)) < e - 1000 and (src == dst).sum() > 10, "the list should hold duplicates and self loops"
    return dict(n=n, e=e, src=src, dst=dst, w=synth.uniform_pm1(seed + 40, (e,), scale=3.0))


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))


# ------------------------------------------------------------------------------------------------ unweighted
def test_unweighted_ref_equals_the_oracle(edges):
    rp, ci = gr.csr_from_coo_ref(edges["src"], edges["dst"], edges["n"])
    orp, oci = oracle.coo_to_csr(edges["src"], edges["dst"], edges["n"])
    assert np.array_equal(rp, orp) and np.array_equal(ci, oci) and ci.dtype == np.int32


@pytest.mark.parametrize("name", ["dupself6", "testgraph_n15", "rmat64"])
def test_unweighted_ref_equals_the_reference_golden(name):
    d = load_case(name)
    rp, ci = gr.csr_from_coo_ref(d["src"], d["dst"], d["n"])
    assert np.array_equal(rows_of(rp), d["ref_ei2"][0]) and np.array_equal(ci, d["ref_ei2"][1])


def test_unweighted_ref_flags_by_definition():
    """The two flags on a list small enough to read: (row, column) pairs in order, kept or collapsed."""
    src = np.array([2, 0, 2, 1, 2, 0, 1], dtype=np.int32)
    dst = np.array([1, 3, 1, 1, 0, 3, 1], dtype=np.int32)
    pairs = lambda rp, ci: list(zip(rows_of(rp).tolist(), ci.tolist()))  # noqa: E731
    assert pairs(*gr.csr_from_coo_ref(src, dst, 5)) == [(0, 3), (2, 0), (2, 1)]
    assert pairs(*gr.csr_from_coo_ref(src, dst, 5, keep_self_loops=True)) == [(0, 3), (1, 1), (2, 0), (2, 1)]
    assert pairs(*gr.csr_from_coo_ref(src, dst, 5, keep_duplicates=True)) == [(0, 3), (0, 3), (2, 0), (2, 1), (2, 1)]
    assert pairs(*gr.csr_from_coo_ref(src, dst, 5, True, True)) == [(0, 3), (0, 3), (1, 1), (1, 1), (2, 0), (2, 1), (2, 1)]
    assert gr.csr_from_coo_ref(src, dst, 5)[0].tolist() == [0, 1, 1, 3, 3, 3]
    for bad_src, bad_dst in (([-1], [0]), ([0], [5]), ([5], [0]), ([0], [-1])):
        with pytest.raises(ValueError):
            gr.csr_from_coo_ref(np.array(bad_src), np.array(bad_dst), 5)
        with pytest.raises(ValueError):
            gr.csr_from_coo_weighted_ref(np.array(bad_src), np.array(bad_dst), np.ones(1), 5)


# ------------------------------------------------------------------------------------------------ weighted
@pytest.mark.parametrize("drop", [False, True], ids=["keep_small", "drop_small"])
@pytest.mark.parametrize("mode,fill", [(gr.DIAG_KEEP, 0.0), (gr.DIAG_STRIP, 0.0), (gr.DIAG_FILL, -1.5), (gr.DIAG_FILL, 0.5)])
def test_weighted_ref_equals_the_oracle(edges, mode, fill, drop):
    n, src, dst, w = edges["n"], edges["src"], edges["dst"], edges["w"]
    want = oracle.coo_to_csr_weighted(src, dst, w, n, diag_mode=mode, diag_value=fill, drop_truncated_zero=drop)
    got = gr.csr_from_coo_weighted_ref(src, dst, w, n, mode, fill, drop_truncated_zero=drop)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(gr.bits(got[2]), gr.bits(want[2]))


@pytest.mark.parametrize("drop", [False, True], ids=["keep_small", "drop_small"])
@pytest.mark.parametrize("mode,fill", [(gr.DIAG_KEEP, 0.0), (gr.DIAG_STRIP, 0.0), (gr.DIAG_FILL, -1.5), (gr.DIAG_FILL, 0.5)])
def test_weighted_dense_definition_equals_the_sort_form_and_the_oracle(mode, fill, drop):
    """n <= 2000: the dense definition, the stable-sort form and the oracle agree, also on the list of special values."""
    n, e = 1500, 40000
    src, dst = synth.rmat_edges(903, n, e)
    w = synth.uniform_pm1(943, (e,), scale=3.0)
    for src, dst, w, n in ((src, dst, w, n), gr.special_weight_list()):
        a = gr.csr_from_coo_weighted_dense_ref(src, dst, w, n, mode, fill, drop_truncated_zero=drop)
        b = gr.csr_from_coo_weighted_ref(src, dst, w, n, mode, fill, drop_truncated_zero=drop)
        o = oracle.coo_to_csr_weighted(src, dst, w, n, diag_mode=mode, diag_value=fill, drop_truncated_zero=drop)
        for x in (b, o):
            assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1]) and np.array_equal(gr.bits(a[2]), gr.bits(x[2]))


@pytest.mark.parametrize("name", ["weighted6", "weighted_rmat64"])
def test_weighted_ref_equals_the_reference_golden(name):
    """The keys tests/test_gpu_parity.py::test_weighted_adjacency_vs_reference_golden reads."""
    d = load_case(name)
    n = d["n"]
    for mode, fill, key in ((gr.DIAG_FILL, 2.5, "w_fill"), (gr.DIAG_STRIP, 0.0, "w_strip")):
        for fn in (gr.csr_from_coo_weighted_ref, gr.csr_from_coo_weighted_dense_ref):
            rp, ci, va = fn(d["src"], d["dst"], d["w"], n, mode, fill, drop_truncated_zero=True)
            assert np.array_equal(rows_of(rp), d["ref_" + key + "_ei"][0]) and np.array_equal(ci, d["ref_" + key + "_ei"][1]), key
            assert np.array_equal(va, d["ref_" + key + "_ea"]), key
    # DIAG_KEEP without the drop: adj->sum(-1) of the reference walks up the row, zeros included
    for fn in (gr.csr_from_coo_weighted_ref, gr.csr_from_coo_weighted_dense_ref):
        rp, ci, va = fn(d["src"], d["dst"], d["w"], n)
        deg = np.zeros(n, dtype=np.float32)
        for i in range(n):
            for p in range(rp[i], rp[i + 1]):
                deg[i] = deg[i] + va[p]
        assert np.array_equal(deg, d["ref_w_deg"].reshape(-1))


def test_weighted_ref_keep_duplicates_by_definition():
    """Every entry of a run stays, in list order, each held to the drop rule by itself; DIAG_FILL still replaces the given loops."""
    src = np.array([1, 0, 1, 2, 1, 2, 0], dtype=np.int32)
    dst = np.array([0, 2, 0, 2, 0, 2, 2], dtype=np.int32)
    w = np.array([3.0, 0.5, -0.25, 9.0, -2.0, 8.0, 6.0], dtype=np.float32)
    out = lambda t: (rows_of(t[0]).tolist(), t[1].tolist(), t[2].tolist())  # noqa: E731
    assert out(gr.csr_from_coo_weighted_ref(src, dst, w, 3, keep_duplicates=True)) == \
        ([0, 0, 1, 1, 1, 2, 2], [2, 2, 0, 0, 0, 2, 2], [0.5, 6.0, 3.0, -0.25, -2.0, 9.0, 8.0])
    assert out(gr.csr_from_coo_weighted_ref(src, dst, w, 3, keep_duplicates=True, drop_truncated_zero=True)) == \
        ([0, 1, 1, 2, 2], [2, 0, 0, 2, 2], [6.0, 3.0, -2.0, 9.0, 8.0])
    assert out(gr.csr_from_coo_weighted_ref(src, dst, w, 3, gr.DIAG_FILL, 1.5, keep_duplicates=True)) == \
        ([0, 0, 0, 1, 1, 1, 1, 2], [0, 2, 2, 0, 0, 0, 1, 2], [1.5, 0.5, 6.0, 3.0, -0.25, -2.0, 1.5, 1.5])
    assert out(gr.csr_from_coo_weighted_ref(src, dst, w, 3)) == ([0, 1, 2], [2, 0, 2], [6.0, -2.0, 8.0])


def test_drop_rule_on_the_special_values_and_nan_on_the_host():
    """dropped iff -1 < w < 1.  For every value but NaN that is `(int)w != 0` on any target; a NaN stays: the restatement keeps it,
    and so does the oracle."""
    v = gr.SPECIAL_WEIGHTS
    assert gr.dropped(v).tolist() == [True, True, True, True, True] + [False] * 9
    assert gr.bits(v)[1] == 0x80000000 and gr.bits(v)[2] == 1 and np.isnan(v[-1])
    assert np.float32(0.99999994) == np.nextafter(np.float32(1), np.float32(0))
    src, dst, w, n = gr.special_weight_list()
    k = len(v)
    for mode in (gr.DIAG_KEEP, gr.DIAG_STRIP):
        rp, ci, va = gr.csr_from_coo_weighted_ref(src, dst, w, n, mode, drop_truncated_zero=True)
        orp, oci, ova = oracle.coo_to_csr_weighted(src, dst, w, n, diag_mode=mode, drop_truncated_zero=True)
        assert np.array_equal(rp, orp) and np.array_equal(ci, oci) and np.array_equal(gr.bits(va), gr.bits(ova))
        per = 3 if mode == gr.DIAG_KEEP else 2
        assert len(ci) == per * (k - 5) and np.isnan(va).sum() == per     # the five small values vanish WITH their earlier entries
        assert np.array_equal(np.diff(rp)[3 * (k - 1): 3 * k], [1, 1, per - 2])   # the NaN's own rows: kept everywhere
    rp, ci, va = gr.csr_from_coo_weighted_ref(src, dst, w, n, keep_duplicates=True, drop_truncated_zero=True)
    assert len(ci) == 6 * k - 3 * 5


# ------------------------------------------------------------------------------------------------ degree block
def test_degree_norm_ref_equals_the_oracle(edges):
    n = edges["n"]
    rp, ci = oracle.coo_to_csr(edges["src"], edges["dst"], n)
    deg = np.diff(rp)
    assert deg.max() >= gr.LONG_ROW and (deg == 0).sum() > 0
    s, norm = gr.degree_norm_ref(rp, ci, n, oracle.powf_table(int(deg.max()) + 2))
    os_, onorm = oracle.degree_norm(rp, ci, n)
    assert np.array_equal(gr.bits(s), gr.bits(os_)) and np.array_equal(gr.bits(norm), gr.bits(onorm))


@pytest.fixture(scope="module")
def norm_case():
    L = gr.norm_row_lengths()
    rp, ci = gr.rows_with_lengths(L, gr.NORM_COLS, gr.NORM_SEED)
    return dict(L=L, rp=rp, ci=ci, s_cols=gr.norm_s_cols(), table=oracle.powf_table(int(L.max()) + 2))


def test_row_length_list_is_where_the_docstring_says(norm_case):
    L, rp, ci = norm_case["L"], norm_case["rp"], norm_case["ci"]
    assert np.array_equal(np.diff(rp), L) and set(gr.REQUIRED_LENGTHS) <= set(L.tolist())
    for i in range(len(L)):
        c = ci[rp[i]:rp[i + 1]]
        assert np.all(np.diff(c) > 0) and (c.size == 0 or (c[0] >= 0 and c[-1] < gr.NORM_COLS))
    long_ = L >= gr.LONG_ROW
    n = len(L)
    assert n % 64 == 37 and long_[n - 1] and gr.NORM_COLS % 64 == 37 and gr.NORM_COLS >= L.max()
    assert long_[:64].sum() >= 5 and long_[0] and long_[63] and long_[62] and long_[17] and long_[18]
    assert not long_[64:128].any() and L[127] == gr.LONG_ROW - 1
    assert long_[128:192].sum() >= 4 and long_[192:256].sum() >= 8 and long_[256:].sum() >= 2
    # chunk tails: a long row's length mod 64 takes 0, 1 and 63 (64 k and 64 k +- 1), and several values in between
    assert {0, 1, 63} <= set((L[long_] % 64).tolist()) and len(set((L[long_] % 64).tolist())) >= 8


def variant_norm(rp, ci, s_cols, s_rows, how):
    """norm with one thing wrong, for the long rows: "ascending" adds from the row's first position up, "chunked" sums every 64
    entries (from the top, as the kernel fetches them) into a partial of its own and then adds the partials."""
    out = np.zeros(len(rp) - 1, dtype=np.float32)
    for i in range(len(rp) - 1):
        v = s_cols[ci[rp[i]:rp[i + 1]]][::-1]          # the right order: last position first
        acc = np.float32(0)
        if how == "ascending":
            for x in v[::-1]:
                acc = acc + x
        else:
            for k in range(0, len(v), 64):
                part = np.float32(0)
                for x in v[k:k + 64]:
                    part = part + x
                acc = acc + part
        out[i] = acc * s_rows[i]
    return out


def test_norm_cases_can_fail(norm_case):
    L, rp, ci, s_cols, table = (norm_case[k] for k in ("L", "rp", "ci", "s_cols", "table"))
    s, norm = gr.degree_norm_ref(rp, ci, len(L), table, s_cols=s_cols)
    assert np.array_equal(s, table[L + 1])
    # the restatement is the plain sequential sum
    seq = np.zeros(len(L), dtype=np.float32)
    for i in range(len(L)):
        acc = np.float32(0)
        for p in range(rp[i + 1] - 1, rp[i] - 1, -1):
            acc = acc + s_cols[ci[p]]
        seq[i] = acc * s[i]
    assert np.array_equal(gr.bits(norm), gr.bits(seq))
    assert np.unique(np.frexp(s_cols)[1]).size >= 12 and not np.any(s_cols == 0), "s_cols should spread over a dozen binades"
    long_ = L >= gr.LONG_ROW
    for how in ("ascending", "chunked"):
        wrong = variant_norm(rp, ci, s_cols, s, how)
        differ = gr.bits(wrong)[long_] != gr.bits(norm)[long_]
        assert differ.mean() >= 0.9, f"{how}: only {differ.sum()} of {long_.sum()} long rows change their bits"
    short = (L > 8) & ~long_
    wrong = variant_norm(rp, ci, s_cols, s, "ascending")
    assert (gr.bits(wrong)[short] != gr.bits(norm)[short]).mean() >= 0.5      # norm_kernel's rows tell the order too
    # the 1057-entry row tells the libm table from a correctly rounded rsqrt
    assert table[1058] != np.float32(1.0 / np.sqrt(np.float64(1058))) and 1057 in L
    assert all(table[k] == np.float32(1.0 / np.sqrt(np.float64(k))) for k in range(1, 1058))
    # with d_s == NULL the rows take the caller's s: another vector than the table's, so a mix-up of the two shows
    assert np.all(s_cols[:len(L)] != s)


def test_weighted_cases_can_fail():
    """The seeded R-MAT list of the GPU test: enough duplicate runs whose first and last weights differ (w = e + 1: all of them),
    and enough whose last weight is dropped while an earlier one would stay."""
    n, e, seed = gr.RMAT
    src, dst = synth.rmat_edges(seed, n, e)
    w2 = synth.uniform_pm1(seed + 40, (e,), scale=3.0)
    key = src.astype(np.int64) * n + dst
    order = np.argsort(key, kind="stable")
    k = key[order]
    start = np.concatenate([[True], k[1:] != k[:-1]])
    run = np.cumsum(start) - 1
    first = order[np.nonzero(start)[0]]
    last = order[np.nonzero(np.concatenate([k[1:] != k[:-1], [True]]))[0]]
    dup = first != last
    assert dup.sum() >= 1000 and (w2[first[dup]] != w2[last[dup]]).sum() >= 1000
    big_earlier = np.zeros(len(first), dtype=bool)
    earlier = np.ones(e, dtype=bool)
    earlier[last] = False                                   # every entry of a run but its last
    np.logical_or.at(big_earlier, run[earlier[order]], np.abs(w2[order][earlier[order]]) >= 1)
    vanish = big_earlier & (np.abs(w2[last]) < 1)
    assert vanish.sum() >= 100
    rp, ci, va = gr.csr_from_coo_weighted_ref(src, dst, w2, n, drop_truncated_zero=True)
    kept = set((rows_of(rp).astype(np.int64) * n + ci).tolist())
    assert not (set(key[last[vanish]].tolist()) & kept), "a pair whose last weight is small vanishes entirely"
    # w = e + 1 names the winner: the value of every entry is its list position + 1, the largest of its pair
    w1 = np.arange(1, e + 1, dtype=np.float32)
    rp, ci, va = gr.csr_from_coo_weighted_ref(src, dst, w1, n)
    pos = va.astype(np.int64) - 1
    assert np.array_equal(src[pos], rows_of(rp)) and np.array_equal(dst[pos], ci) and np.array_equal(np.sort(pos), np.sort(last))
