"""CPU checks of the graph readout's restatement (tests/pool_ref.py), of the inputs the GPU test shares with it, and of what the C-ABI
decides without a device: the restatement against hand-written expectations; proof that the shared inputs tell the contract's order
from its neighbours (chunk length 128, a descending walk, chunks counted from global row 0, a reciprocal multiply for the mean);
every GNNX_ERR_INVALID_ARG case of the header; the workspace query against the header's formula."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import pool_ref
from tests.helpers import ROOT, pkg  # noqa: F401
from tests.pool_ref import T, pool_bwd, pool_fwd

INVALID, OK = -1, 0
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


# ---- the restatement against hand-written expectations ---------------------------------------------------------------------------------
def test_sum_is_one_ascending_chain_per_chunk():
    # float32 near 1e8 has an ulp of 8: 1e8 + 4 is a tie and rounds to the even 1e8, 1e8 + 8 is exact
    X = np.array([[1e8], [4.0], [4.0]], dtype=f32)
    Y, arg = pool_fwd([0, 3], X, "sum")
    assert arg is None and Y[0, 0] == f32(1e8)                                  # ((0 + 1e8) + 4) + 4: both 4s are lost
    assert pool_fwd([0, 3], X, "sum", descending=True)[0][0, 0] == f32(1e8) + f32(8)   # (4 + 4) + 1e8
    assert bits(pool_fwd([0, 1], np.array([[-0.0]], dtype=f32), "sum")[0])[0, 0] == 0   # the chain starts at +0: +0 + -0 = +0
    assert bits(pool_fwd([0, 0, 0], np.zeros((0, 2), dtype=f32), "sum")[0]).tolist() == [[0, 0], [0, 0]]   # no rows at all


def test_sum_chunks_count_from_the_segments_own_first_row():
    # a segment of 2 T + 1 rows that starts at row 3: chunks [3, 3 + T), [3 + T, 3 + 2 T), [3 + 2 T, 3 + 2 T + 1)
    n = 3 + 2 * T + 1
    X = np.zeros((n, 1), dtype=f32)
    X[3 + T - 1] = 4.0          # the last row of chunk 0
    X[3 + T] = 4.0              # the first row of chunk 1
    X[3 + T + 1] = 1e8          # chunk 1: (0 + 4) + 1e8 = 1e8, the 4 is lost
    Y, _ = pool_fwd([0, 3, n], X, "sum")
    assert Y[0, 0] == 0 and Y[1, 0] == f32(1e8)                                  # (c_0 + c_1) + c_2 = (4 + 1e8) + 0 = 1e8
    # one chain over the whole segment, or chunks cut at the global rows 256 and 512, keep both 4s: (4 + 4) + 1e8
    assert pool_fwd([0, 3, n], X, "sum", chunk=4 * T)[0][1, 0] == f32(1e8) + f32(8)
    assert pool_fwd([0, 3, n], X, "sum", global_chunks=True)[0][1, 0] == f32(1e8) + f32(8)
    # the same segment anywhere else has the same bits
    X2 = np.concatenate([np.ones((100, 1), dtype=f32), X[3:]])
    assert pool_fwd([0, 100, 100 + 2 * T + 1], X2, "sum")[0][1, 0] == f32(1e8)


def test_mean_is_one_division():
    X = np.array([[1.0], [1.0], [1.0], [7.0]], dtype=f32)
    Y, _ = pool_fwd([0, 3, 3, 4], X, "mean")
    assert Y[0, 0] == f32(3.0) / f32(3.0) and Y[2, 0] == f32(7)
    assert bits(Y)[1, 0] == 0                                   # the empty segment: +0, no 0 / 0
    X = np.full((3, 1), 5.0, dtype=f32)
    assert pool_fwd([0, 3], X, "mean")[0][0, 0] == f32(15) / f32(3) == f32(5)
    assert pool_fwd([0, 3], X, "mean", reciprocal_mean=True)[0][0, 0] == f32(15) * (f32(1) / f32(3))


def test_max_first_winner_signed_zero_and_neg_inf():
    ninf = -np.inf
    X = np.array([[1, -0.0, ninf, 2],
                  [2, 0.0, ninf, 2],
                  [2, -0.0, ninf, 1],
                  [9, 9, 9, 9],
                  [0.0, 5, ninf, -1]], dtype=f32)
    Y, arg = pool_fwd([0, 3, 3, 4, 5], X, "max")
    assert arg.dtype == np.int32
    assert arg[0].tolist() == [1, 0, 0, 0]                      # the first of the ties; -0 at row 0 beats the later +0; all -inf: row 0
    assert bits(Y[0]).tolist() == bits(np.array([2, -0.0, ninf, 2], dtype=f32)).tolist()
    assert arg[1].tolist() == [-1] * 4 and bits(Y[1]).tolist() == [0] * 4     # empty: +0 and -1
    assert arg[2].tolist() == [3] * 4 and arg[3].tolist() == [4] * 4           # ABSOLUTE rows


def test_backward_forms_and_both_betas():
    segptr = [0, 3, 3, 4]
    G = np.array([[3.0, 6.0], [100.0, 100.0], [5.0, 7.0]], dtype=f32)
    nan = np.full((4, 2), np.nan, dtype=f32)
    d = pool_bwd(segptr, G, "sum", dX=nan, beta=0.0)
    assert d.tolist() == [[3, 6], [3, 6], [3, 6], [5, 7]]        # the NaN vanished: dX is not read; the empty segment's G goes nowhere
    d = pool_bwd(segptr, G, "mean", beta=0.0)
    assert np.array_equal(d, np.array([[1, 2], [1, 2], [1, 2], [5, 7]], dtype=f32))
    G3 = np.array([[1.0, 1.0], [0, 0], [1, 1]], dtype=f32)
    assert pool_bwd(segptr, G3, "mean")[0, 0] == f32(1) / f32(3)
    arg = np.array([[2, 0], [-1, -1], [3, 3]], dtype=np.int32)
    d = pool_bwd(segptr, G, "max", arg=arg, beta=0.0)
    assert d.tolist() == [[0, 6], [0, 0], [3, 0], [5, 7]]
    old = np.array([[1e8, 1], [1, 1], [1, 1], [0.5, 0.5]], dtype=f32)
    d = pool_bwd(segptr, G, "sum", dX=old, beta=1.0)
    assert d[0, 0] == f32(1e8) + f32(3) and d[3].tolist() == [5.5, 7.5]       # one rounded add
    d = pool_bwd(segptr, G, "max", arg=arg, dX=old, beta=1.0)
    assert d.tolist() == [[1e8, 7], [1, 1], [4, 1], [5.5, 7.5]]


def test_position_independence_of_the_restatement():
    segptr, X = pool_ref.segment_table().astype(np.int64), pool_ref.sum_values()[:, :3]
    Y, _ = pool_fwd(segptr, X, "sum")
    for b in np.argsort(-np.diff(segptr))[:4]:
        s, e = segptr[b], segptr[b + 1]
        alone, _ = pool_fwd([0, e - s], np.ascontiguousarray(X[s:e]), "sum")
        assert np.array_equal(bits(alone[0]), bits(Y[b]))


# ---- the shared inputs discriminate ------------------------------------------------------------------------------------------------------
def test_segment_table_has_the_lengths_the_gpu_test_relies_on():
    segptr = pool_ref.segment_table().astype(np.int64)
    lens = np.diff(segptr)
    assert segptr[0] == 0 and (lens >= 0).all() and 18_000 <= segptr[-1] <= 22_000
    assert lens[0] == 0 and lens[-1] == 0
    assert any((lens[i:i + 3] == 0).all() for i in range(len(lens) - 2))
    for ln in (1, 2, 63, 64, 65) + pool_ref.LONG:
        assert (lens == ln).any(), ln
    short_run = (lens >= 1) & (lens <= 3)
    assert max(len(r) for r in "".join("x" if v else " " for v in short_run).split()) >= 300
    for b in np.nonzero(lens > T - 2)[0][:len(pool_ref.LONG)]:
        assert 0 < lens[b - 1] < T and 0 < lens[b + 1] < T       # short neighbours on both sides
    # a global tile with the tail of one long segment, whole short ones and the head of another
    long_b = np.nonzero(lens > T)[0]
    found = False
    for t in range(int(segptr[-1]) // T + 1):
        lo, hi = t * T, (t + 1) * T
        tails = [b for b in long_b if segptr[b] < lo < segptr[b + 1] <= hi]
        heads = [b for b in long_b if lo < segptr[b] < hi < segptr[b + 1]]
        whole = [b for b in range(len(lens)) if 0 < lens[b] <= T and lo <= segptr[b] and segptr[b + 1] <= hi]
        found |= bool(tails and heads and whole)
    assert found


@pytest.mark.parametrize("variant", [dict(chunk=128), dict(descending=True), dict(global_chunks=True)])
def test_sum_inputs_tell_the_contract_from_a_neighbouring_order(variant):
    segptr = pool_ref.segment_table().astype(np.int64)
    X = pool_ref.sum_values()[:, :8]
    Y = pool_ref.reference("sum")[0][:, :8]
    assert np.array_equal(bits(Y), bits(pool_fwd(segptr, X, "sum")[0]))         # columns are independent chains
    Yv, _ = pool_fwd(segptr, X, "sum", **variant)
    long_segments = np.diff(segptr) > T
    differ = (bits(Y) != bits(Yv)).any(axis=1)
    assert (differ & long_segments).any(), f"{variant}: no segment longer than T tells it from the contract"


def test_mean_inputs_tell_a_reciprocal_multiply_from_the_division():
    segptr = pool_ref.segment_table().astype(np.int64)
    X = pool_ref.sum_values()[:, :8]
    Y = pool_ref.reference("mean")[0][:, :8]
    Yv, _ = pool_fwd(segptr, X, "mean", reciprocal_mean=True)
    assert (bits(Y) != bits(Yv)).any()


def test_max_inputs_are_full_of_ties():
    segptr = pool_ref.segment_table().astype(np.int64)
    X = pool_ref.max_values()
    Y, arg = pool_ref.reference("max")
    b = pool_ref.all_neg_inf_segment()
    assert np.isneginf(Y[b]).all() and (arg[b] == segptr[b]).all()
    lens = np.diff(segptr)
    ne = lens > 0
    assert (arg[ne] >= segptr[:-1][ne, None]).all() and (arg[ne] < segptr[1:][ne, None]).all() and (arg[~ne] == -1).all()
    big = int(np.argmax(lens))
    ties = (X[segptr[big]:segptr[big + 1]] == Y[big]).sum(axis=0)
    assert ties.min() > 1                                                      # the winner is never alone
    zero_wins = (Y == 0) & ne[:, None]
    assert (bits(Y)[zero_wins] == 0).any() and (bits(Y)[zero_wins] != 0).any()  # +0 and -0 both win somewhere
    assert (arg[big] > segptr[big] + T).any()                                  # a winner outside the first chunk


# ---- what the library decides without a device ---------------------------------------------------------------------------------------------
def test_argument_validation_without_device(capi):
    L = capi.lib()
    p = C.c_void_p(256)          # never dereferenced: every case is refused before any device call
    ws = C.c_size_t(1 << 20)

    def fwd(op=0, n_seg=2, n_rows=10, F=4, segptr=p, X=p, ldx=4, Y=p, ldy=4, arg=p, lda=4):
        return L.gnnx_segment_pool_f32(op, n_seg, n_rows, F, segptr, X, ldx, Y, ldy, arg, lda, p, ws, None)

    def bwd(op=0, n_seg=2, n_rows=10, F=4, segptr=p, arg=p, lda=4, G=p, ldg=4, beta=0.0, dX=p, ldx=4):
        return L.gnnx_segment_pool_bwd_f32(op, n_seg, n_rows, F, segptr, arg, lda, G, ldg, beta, dX, ldx, None)

    for call in (fwd, bwd):
        assert call(n_seg=-1) == INVALID and call(n_rows=-1) == INVALID and call(F=-1) == INVALID      # negative sizes
        assert call(op=3) == INVALID and call(op=-1) == INVALID                                     # op outside the enum
        assert call(ldx=3) == INVALID                                                               # ld < n_feat
        assert call(n_seg=0, n_rows=5) == INVALID                                                   # rows in no segment
        assert call(segptr=None) == INVALID and b"null" in L.gnnx_last_error()                      # null pointers
        assert call(n_seg=0, n_rows=0) == OK and call(F=0) == OK                                    # nothing to do, nothing written
    assert fwd(ldy=3) == INVALID and fwd(op=2, lda=3) == INVALID
    assert fwd(X=None) == INVALID and fwd(Y=None) == INVALID
    assert bwd(ldg=3) == INVALID and bwd(op=2, lda=3) == INVALID
    assert bwd(G=None) == INVALID and bwd(dX=None) == INVALID
    assert bwd(op=2, arg=None) == INVALID                                                           # MAX backward needs the arg
    for beta in (0.5, -1.0, 2.0, float("nan")):
        assert bwd(beta=beta) == INVALID
    # a workspace that is NULL or too small: refused before any device call as well
    need = C.c_size_t(0)
    assert L.gnnx_segment_pool_workspace(2, 10, 4, C.byref(need)) == OK
    WORKSPACE = L.gnnx_segment_pool_f32(0, 2, 10, 4, p, p, 4, p, 4, None, 0, None, 0, None)
    assert WORKSPACE not in (OK, INVALID) and b"workspace" in L.gnnx_last_error()
    assert L.gnnx_segment_pool_f32(0, 2, 10, 4, p, p, 4, p, 4, None, 0, p, need.value - 1, None) == WORKSPACE


def test_workspace_query(capi):
    L = capi.lib()
    assert L.gnnx_segment_pool_workspace(1, 1, 1, None) == INVALID
    b = C.c_size_t(0)
    assert L.gnnx_segment_pool_workspace(-1, 1, 1, C.byref(b)) == INVALID
    assert L.gnnx_segment_pool_workspace(1, -1, 1, C.byref(b)) == INVALID
    assert L.gnnx_segment_pool_workspace(1, 1, -1, C.byref(b)) == INVALID

    def q(n_seg, n_rows, F):
        assert L.gnnx_segment_pool_workspace(n_seg, n_rows, F, C.byref(b)) == OK
        return b.value

    for n_rows in (0, 1, T - 1, T, T + 1, 20_000, 1_000_000, 2 ** 31 - 1):
        for F in (0, 1, 4, 128, 516):
            for n_seg in (0, 1, 50_000):
                assert q(n_seg, n_rows, F) == pool_ref.workspace_bytes(n_rows, F)
    sizes = (0, 1, 255, 256, 257, 1000, 100_000)
    for a0, a1 in zip(sizes[:-1], sizes[1:]):          # monotone in each size
        assert q(a0, 1000, 64) <= q(a1, 1000, 64)
        assert q(10, a0, 64) <= q(10, a1, 64)
        assert q(10, 1000, a0) <= q(10, 1000, a1)
    assert q(8, 1_000_000, 128) < q(8, 2_000_000, 128) and q(8, 1_000_000, 128) < q(8, 1_000_000, 256)
