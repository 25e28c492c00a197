"""The graph build held to its restatement (run with -m gpu on an MI355X): gnnx_csr_from_coo under all four flag values,
gnnx_csr_from_coo_weighted under its whole 3 x 2 x 2 grid of diagonal mode, GNNX_CSR_KEEP_DUPLICATES and
GNNX_CSR_DROP_TRUNCATED_ZERO, gnnx_degree_norm_f32 in every pointer mode on a CSR whose row lengths sit on every edge of its two
norm kernels, and gnnx_equal_i32.

The reference is tests/graph_ref.py (NumPy; pinned to the oracle and the compiled reference's golden vectors by
tests/test_graph_ref_cpu.py, which also proves that these cases tell a wrong summation order, a wrong hand-over between the two norm
kernels and a wrong winner of a duplicate run from the right ones).  Everything is integer work or strictly ordered float32, so every
comparison is equality; float values are compared as bit patterns, so that -0.0 and NaN count."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle
from tests import graph_ref as gr
from tests.helpers import synth

pytestmark = pytest.mark.gpu

INDEX_RANGE, WORKSPACE, INVALID_ARG = -3, -4, -1      # include/gnnx.h
RANGE_MESSAGE = "invalid input, max value in edge_index should be less than the number of nodes from x"
SENTINEL_BITS = 0x7FC0BEEF                           # a NaN no sum produces: an output element that was never written


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


def i32(*v):
    return np.array(v, dtype=np.int32).reshape(-1)


# ================================================================================================ unweighted
def _rmat():
    n, e, seed = gr.RMAT
    return synth.rmat_edges(seed, n, e) + (n,)


def _seeded(n_rows, n_cols, e, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_rows, e).astype(np.int32), rng.integers(0, n_cols, e).astype(np.int32)


def _wide():
    """n = 70 001, 5000 edges: ids above 2^16, the last vertex used, and a rowptr whose binary searches mostly hit empty rows."""
    src, dst = _seeded(70001, 70001, 5000, 11)
    src[:4], dst[:4] = (70000, 65536, 65537, 70000), (65535, 70000, 65537, 70000)
    src[10:20], dst[10:20] = src[20:30], dst[20:30]          # some duplicates
    return src, dst, 70001


def _hand_written():
    """Duplicates, self loops, empty first and last rows (0 and 8), vertex n - 1 used as a column, a duplicated self loop."""
    return i32(3, 1, 3, 5, 1, 7, 3, 5, 2, 7, 1, 5), i32(8, 2, 8, 5, 2, 1, 0, 5, 8, 7, 1, 4), 9


UNWEIGHTED_CASES = {
    "hand_written": _hand_written,
    "n1": lambda: (i32(0, 0, 0), i32(0, 0, 0), 1),
    "E1": lambda: (i32(2), i32(4), 6),
    "E1_self_loop": lambda: (i32(2), i32(2), 6),
    "E256": lambda: _seeded(50, 50, 256, 12) + (50,),
    "E257": lambda: _seeded(50, 50, 257, 13) + (50,),
    "only_self_loops": lambda: (i32(4, 0, 4, 9, 2, 0), i32(4, 0, 4, 9, 2, 0), 10),
    "one_edge_300_times": lambda: (np.full(300, 6, dtype=np.int32), np.full(300, 3, dtype=np.int32), 8),
    # the last key in sorted order: kept (unique, no sentinel behind it) / dropped as the second of a run / dropped as a self loop,
    # which the default flags turn into the sentinel that sorts last -- nnz = pos[last] + flag[last] either way
    "last_sorted_kept": lambda: (i32(5, 0, 2, 5, 2), i32(4, 3, 1, 2, 1), 6),
    "last_sorted_duplicate": lambda: (i32(5, 0, 5, 2, 5), i32(4, 3, 4, 1, 2), 6),
    "last_sorted_self_loop": lambda: (i32(5, 0, 3, 2, 5), i32(5, 3, 3, 1, 2), 6),
    "n70001": _wide,
    "rmat3001": _rmat,
}


@pytest.mark.parametrize("flags", gr.UNWEIGHTED_FLAGS)
@pytest.mark.parametrize("case", list(UNWEIGHTED_CASES))
def test_csr_from_coo_every_flag(env, case, flags):
    src, dst, n = UNWEIGHTED_CASES[case]()
    rp, ci = gr.csr_from_coo_ref(src, dst, n, bool(flags & gr.KEEP_SELF_LOOPS), bool(flags & gr.KEEP_DUPLICATES))
    grp, gci = env["ops"].CsrGraph.csr_from_coo(dev(env, src), dev(env, dst), n, flags=flags)
    assert gci.numel() == len(ci), f"nnz {gci.numel()}, expected {len(ci)}"
    assert np.array_equal(host(grp), rp) and np.array_equal(host(gci), ci)
    if case == "only_self_loops" and flags in (0, gr.KEEP_DUPLICATES):
        assert len(src) > 0 and gci.numel() == 0 and not host(grp).any()


@pytest.mark.parametrize("flags", (gr.KEEP_SELF_LOOPS, gr.KEEP_SELF_LOOPS | gr.KEEP_DUPLICATES))
def test_csr_from_coo_rectangular_rows_keep_the_diagonal(env, flags):
    """The shard-style use: rows are local ids in [0, 500), columns global ids in [0, 3001); a row id that equals a column id is an
    ordinary entry."""
    src, dst = _seeded(500, 3001, 20000, 14)
    assert (src == dst).sum() >= 3
    rp, ci = gr.csr_from_coo_ref(src, dst, 3001, True, bool(flags & gr.KEEP_DUPLICATES))
    grp, gci = env["ops"].CsrGraph.csr_from_coo(dev(env, src), dev(env, dst), 3001, flags=flags)
    assert gci.numel() == len(ci) and np.array_equal(host(grp), rp) and np.array_equal(host(gci), ci)
    assert rp[500] == len(ci)


def _raw_csr_from_coo(env, src, dst, n, ws, ws_bytes):
    torch, capi = env["torch"], env["capi"]
    E = int(src.numel())
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=env["dev"])
    colidx = torch.empty(max(E, 1), dtype=torch.int32, device=env["dev"])
    nnz = C.c_int64(-1)
    capi.call("gnnx_csr_from_coo", C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), E, n, 0, C.c_void_p(rowptr.data_ptr()),
              C.c_void_p(colidx.data_ptr()), C.byref(nnz), C.c_void_p(ws.data_ptr()), ws_bytes, None)
    return host(rowptr), host(colidx[: nnz.value])


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bad", ["src=-1", "dst=n", "src=n"])
def test_csr_from_coo_endpoint_out_of_range(env, bad, where):
    """One bad endpoint at either end of an otherwise valid list of 300: status -3 with the reference's message, and the next call
    on the SAME workspace succeeds (the device-side flag is reset per call)."""
    torch, capi = env["torch"], env["capi"]
    n = 40
    src, dst = _seeded(n, n, 300, 15)
    good = gr.csr_from_coo_ref(src, dst, n)
    bsrc, bdst = src.copy(), dst.copy()
    e = 0 if where == "first" else 299
    if bad == "src=-1":
        bsrc[e] = -1
    elif bad == "dst=n":
        bdst[e] = n
    else:
        bsrc[e] = n
    with pytest.raises(ValueError):
        gr.csr_from_coo_ref(bsrc, bdst, n)
    need = capi.csr_from_coo_workspace(300, n)
    ws = torch.empty(need, dtype=torch.uint8, device=env["dev"])
    with pytest.raises(capi.GnnxError) as err:
        _raw_csr_from_coo(env, dev(env, bsrc), dev(env, bdst), n, ws, need)
    assert err.value.status == INDEX_RANGE and RANGE_MESSAGE in str(err.value)
    rp, ci = _raw_csr_from_coo(env, dev(env, src), dev(env, dst), n, ws, need)
    assert np.array_equal(rp, good[0]) and np.array_equal(ci, good[1])


def test_csr_from_coo_workspace_one_byte_short(env):
    torch, capi = env["torch"], env["capi"]
    n = 40
    src, dst = _seeded(n, n, 300, 15)
    need = capi.csr_from_coo_workspace(300, n)
    ws = torch.empty(need, dtype=torch.uint8, device=env["dev"])
    with pytest.raises(capi.GnnxError) as err:
        _raw_csr_from_coo(env, dev(env, src), dev(env, dst), n, ws, need - 1)
    assert err.value.status == WORKSPACE
    good = gr.csr_from_coo_ref(src, dst, n)
    rp, ci = _raw_csr_from_coo(env, dev(env, src), dev(env, dst), n, ws, need)
    assert np.array_equal(rp, good[0]) and np.array_equal(ci, good[1])


# ================================================================================================ weighted
def _weighted_flags(ops, keep_dup, drop):
    return (ops.CSR_KEEP_DUPLICATES if keep_dup else 0) | (ops.CSR_DROP_TRUNCATED_ZERO if drop else 0)


def _check_weighted(env, src, dst, w, n, mode, fill, keep_dup, drop, what):
    ops = env["ops"]
    rp, ci, va = gr.csr_from_coo_weighted_ref(src, dst, w, n, mode, fill, keep_duplicates=keep_dup, drop_truncated_zero=drop)
    grp, gci, gva = ops.csr_from_coo_weighted(dev(env, src), dev(env, dst), dev(env, w), n, diag_mode=mode, diag_value=fill,
                                              flags=_weighted_flags(ops, keep_dup, drop))
    assert gci.numel() == len(ci) and gva.numel() == len(ci), f"{what}: nnz {gci.numel()}, expected {len(ci)}"
    assert np.array_equal(host(grp), rp) and np.array_equal(host(gci), ci), what
    differ = np.nonzero(gr.bits(host(gva)) != gr.bits(va))[0]
    assert differ.size == 0, f"{what}: {differ.size} values differ, first at entry {differ[0]}: {host(gva)[differ[0]]} != {va[differ[0]]}"
    return rp, ci, va


GRID_IDS = [f"{('keep', 'strip', 'fill')[m]}-{'dups' if kd else 'last'}-{'drop' if dz else 'all'}" for m, kd, dz in gr.WEIGHTED_GRID]


@pytest.mark.parametrize("mode,keep_dup,drop", gr.WEIGHTED_GRID, ids=GRID_IDS)
def test_weighted_grid_rmat(env, mode, keep_dup, drop):
    """w = e + 1 names the list position of every surviving entry (nothing is below 1); under the drop flag a second weight vector
    in (-3, 3) makes a third of the entries vanish, whole pairs with them."""
    n, e, seed = gr.RMAT
    src, dst = synth.rmat_edges(seed, n, e)
    fill = 2.5
    rp, ci, va = _check_weighted(env, src, dst, np.arange(1, e + 1, dtype=np.float32), n, mode, fill, keep_dup, drop, "w = e + 1")
    if not keep_dup and mode == gr.DIAG_KEEP:
        pos = va.astype(np.int64) - 1              # the restated winner is the last list position of its pair
        key = src.astype(np.int64) * n + dst
        last = {}
        for p, k in enumerate(key.tolist()):
            last[k] = p
        assert np.array_equal(np.sort(pos), np.sort(np.fromiter(last.values(), dtype=np.int64)))
    if drop:
        w2 = synth.uniform_pm1(seed + 40, (e,), scale=3.0)
        _, ci2, _ = _check_weighted(env, src, dst, w2, n, mode, fill, keep_dup, drop, "uniform(-3, 3)")
        assert len(ci2) < 0.8 * len(ci)


@pytest.mark.parametrize("mode,keep_dup,drop", gr.WEIGHTED_GRID, ids=GRID_IDS)
def test_weighted_grid_special_values(env, mode, keep_dup, drop):
    """0.0, -0.0, the smallest denormal, +-(1 - 2^-24), +-1, +-2^31, +-3e38, +-inf and NaN, each alone, as the last of a run and as
    a self loop.  Under GNNX_CSR_DROP_TRUNCATED_ZERO an entry is dropped iff -1 < w < 1: NaN stays."""
    src, dst, w, n = gr.special_weight_list()
    for fill in (2.5, float("nan")) if mode == gr.DIAG_FILL else (0.0,):
        _, _, va = _check_weighted(env, src, dst, w, n, mode, fill, keep_dup, drop, f"fill {fill}")
        if drop:
            assert not np.any(gr.dropped(va)) and np.isnan(va).sum() >= 2


def test_weighted_diag_fill_corners(env):
    ops = env["ops"]
    n = 37
    none = np.zeros(0, dtype=np.int32)
    # E = 0 with DIAG_FILL: n diagonal entries
    rp, ci, va = _check_weighted(env, none, none, np.zeros(0, dtype=np.float32), n, gr.DIAG_FILL, 3.0, False, False, "E = 0")
    assert np.array_equal(rp, np.arange(n + 1)) and np.array_equal(ci, np.arange(n)) and np.all(va == 3.0)
    src, dst = _seeded(n, n, 400, 16)
    src[:5], dst[:5] = (3, 9, 3, 36, 0), (3, 9, 3, 36, 0)         # given self loops, one of them twice
    w = np.arange(1, 401, dtype=np.float32)
    # diag_value 0.5 under the drop flag: no diagonal at all
    rp, ci, va = _check_weighted(env, src, dst, w, n, gr.DIAG_FILL, 0.5, False, True, "fill 0.5, drop")
    assert not np.any(np.repeat(np.arange(n), np.diff(rp)) == ci)
    # diag_value 0.0 without it: n explicit zeros
    rp, ci, va = _check_weighted(env, src, dst, w, n, gr.DIAG_FILL, 0.0, False, False, "fill 0.0")
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    assert diag.sum() == n and not gr.bits(va[diag]).any()
    rp, ci, va = _check_weighted(env, src, dst, w, n, gr.DIAG_FILL, -0.0, False, False, "fill -0.0")
    assert np.all(gr.bits(va[np.repeat(np.arange(n), np.diff(rp)) == ci]) == 0x80000000)
    # DIAG_FILL with KEEP_DUPLICATES: the given self loops are gone, one filled entry per vertex remains
    rp, ci, va = _check_weighted(env, src, dst, w, n, gr.DIAG_FILL, -9.0, True, False, "fill, keep duplicates")
    diag = np.repeat(np.arange(n), np.diff(rp)) == ci
    assert diag.sum() == n and np.all(va[diag] == -9.0) and len(ci) == n + int((src != dst).sum())
    assert ops.DIAG_FILL == gr.DIAG_FILL and ops.DIAG_STRIP == gr.DIAG_STRIP and ops.DIAG_KEEP == gr.DIAG_KEEP


# ================================================================================================ degree block
@pytest.fixture(scope="module")
def norm_case(env):
    L = gr.norm_row_lengths()
    rp, ci = gr.rows_with_lengths(L, gr.NORM_COLS, gr.NORM_SEED)
    return dict(L=L, n=len(L), rp=rp, ci=ci, s_cols=gr.norm_s_cols(), table=oracle.powf_table(int(L.max()) + 2),
                rp_d=dev(env, rp.astype(np.int32)), ci_d=dev(env, ci))


def _degree_norm(env, rp_d, ci_d, n_rows, want_s, s_cols, want_norm=True):
    """gnnx_degree_norm_f32 with outputs pre-filled by a sentinel bit pattern -> (s bits, norm bits), None where not asked for."""
    torch, capi = env["torch"], env["capi"]
    fill = lambda k: dev(env, np.full(k, SENTINEL_BITS, dtype=np.uint32).view(np.float32))  # noqa: E731
    s = fill(n_rows) if want_s else None
    norm = fill(n_rows) if want_norm else None
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    capi.call("gnnx_degree_norm_f32", p(rp_d), p(ci_d), n_rows, p(s), p(s_cols), p(norm), None)
    torch.cuda.synchronize()
    return tuple(None if t is None else gr.bits(host(t)) for t in (s, norm))


def _assert_rows(got_bits, want, what):
    assert not np.any(got_bits == SENTINEL_BITS), f"{what}: rows {np.nonzero(got_bits == SENTINEL_BITS)[0][:8]} were never written"
    bad = np.nonzero(got_bits != gr.bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, the first: {bad[:8]}"


def test_degree_norm_callers_s(env, norm_case):
    """d_s == NULL: rows and columns both take the caller's vector (longer than n_rows).  The seeded s spreads over a dozen binades,
    so the order of the additions and any partial sum show in the bits (tests/test_graph_ref_cpu.py::test_norm_cases_can_fail)."""
    c = norm_case
    _, norm = gr.degree_norm_ref(c["rp"], c["ci"], c["n"], c["table"], s_cols=c["s_cols"], s_rows=c["s_cols"])
    s_bits, got = _degree_norm(env, c["rp_d"], c["ci_d"], c["n"], False, dev(env, c["s_cols"]))
    assert s_bits is None
    _assert_rows(got, norm, "norm")


def test_degree_norm_local_rows_and_halo_columns(env, norm_case):
    """d_s written for the rows, a longer d_s_cols for the columns (the [local | halo] call of a shard)."""
    c = norm_case
    s, norm = gr.degree_norm_ref(c["rp"], c["ci"], c["n"], c["table"], s_cols=c["s_cols"])
    got_s, got = _degree_norm(env, c["rp_d"], c["ci_d"], c["n"], True, dev(env, c["s_cols"]))
    assert np.array_equal(s, c["table"][c["L"] + 1])
    _assert_rows(got_s, s, "s")
    _assert_rows(got, norm, "norm")
    # d_norm == NULL: s alone
    got_s, none = _degree_norm(env, c["rp_d"], c["ci_d"], c["n"], True, None, want_norm=False)
    assert none is None
    _assert_rows(got_s, s, "s without norm")


def test_degree_norm_square(env, norm_case):
    """d_s written and used for both sides: the CSR padded with empty rows to n_cols rows."""
    c = norm_case
    n = gr.NORM_COLS
    rp = np.concatenate([c["rp"], np.full(n - c["n"], c["rp"][-1], dtype=np.int64)])
    s, norm = gr.degree_norm_ref(rp, c["ci"], n, c["table"])
    assert np.array_equal(s, c["table"][np.diff(rp) + 1]) and np.all(s[c["n"]:] == 1.0) and not norm[c["n"]:].any()
    got_s, got = _degree_norm(env, dev(env, rp.astype(np.int32)), c["ci_d"], n, True, None)
    _assert_rows(got_s, s, "s")
    _assert_rows(got, norm, "norm")


def test_degree_norm_empty_and_null_arguments(env, norm_case):
    torch, capi = env["torch"], env["capi"]
    c = norm_case
    # n_rows = 0: nothing is read or written
    capi.call("gnnx_degree_norm_f32", None, None, 0, None, None, None, None)
    s_bits, got = _degree_norm(env, c["rp_d"], c["ci_d"], 0, True, None)
    assert s_bits.size == 0 and got.size == 0
    # colidx == NULL with nnz == 0 is fine: s = 1, norm = 0 everywhere
    zero_rp = torch.zeros(101, dtype=torch.int32, device=env["dev"])
    s_bits, got = _degree_norm(env, zero_rp, None, 100, True, None)
    _assert_rows(s_bits, np.ones(100, dtype=np.float32), "s of an empty graph")
    _assert_rows(got, np.zeros(100, dtype=np.float32), "norm of an empty graph")
    # colidx == NULL with nnz > 0 is refused before any entry is read
    with pytest.raises(capi.GnnxError) as err:
        _degree_norm(env, c["rp_d"], None, c["n"], True, None)
    assert err.value.status == INVALID_ARG
    with pytest.raises(capi.GnnxError) as err:     # neither d_s nor d_s_cols
        _degree_norm(env, c["rp_d"], c["ci_d"], c["n"], False, None)
    assert err.value.status == INVALID_ARG


# ================================================================================================ gnnx_equal_i32
def test_equal_i32(env):
    torch, capi = env["torch"], env["capi"]

    def equal(a, b, n):
        out = C.c_int(-1)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        capi.call("gnnx_equal_i32", p(a), p(b), n, C.byref(out), None)
        return out.value

    a = dev(env, np.arange(257, dtype=np.int32) * 3 - 100)
    b = a.clone()
    assert equal(None, None, 0) == 1 and equal(a, b, 0) == 1
    assert equal(a, a, 257) == 1
    assert equal(a, b, 257) == 1 and equal(a, b, 256) == 1 and equal(a, b, 1) == 1
    first = a.clone()
    first[0] += 1
    assert equal(a, first, 257) == 0 and equal(a, first, 1) == 0
    last = a.clone()
    last[256] -= 1
    assert equal(a, last, 257) == 0 and equal(a, last, 256) == 1      # the differing element lies behind n
    with pytest.raises(capi.GnnxError) as err:
        equal(a, None, 257)
    assert err.value.status == INVALID_ARG
    torch.cuda.synchronize()
