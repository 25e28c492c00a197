"""The comparison helpers of tests/test_gpu_large_offsets.py can fail (no GPU needed): each is fed a correct array and a corrupted copy
-- a row dropped from a reduction, two rows swapped, a 256-row tile shifted by one row, an element off by one ulp (rounding legs: must
pass) and by 2e-5 of the scale (must fail) -- and must report the corruption.  And the documented blind spot of the suite's
condition-aware bar is pinned as a fact: at n = 1e7 rows it does NOT see whole rows missing from dH^T.X, the exact leg does."""
import numpy as np
import pytest
import torch

from tests import test_gpu_large_offsets as big
from tests.helpers import (RTOL, assert_close, assert_rows_close, assert_rows_equal, assert_small_equal, chunked_sum, dma_tail_round,
                           fill_small_ints, row_chunks, rows_mismatch, sample_rows, take_rows)

STEP = 1000   # small chunks: every helper crosses chunk borders


def small_ints(shape, seed):
    return fill_small_ints(torch.empty(shape, dtype=torch.float32), torch.Generator().manual_seed(seed), step=STEP)


def test_integer_fill_is_seeded_chunked_and_in_range():
    a, b = small_ints((2500, 8), 3), small_ints((2500, 8), 3)
    assert torch.equal(a, b) and set(a.unique().tolist()) == {-1.0, 0.0, 1.0}
    wide = torch.full((2500, 32), 7.0)
    fill_small_ints(wide[:, 4:12], torch.Generator().manual_seed(3), step=STEP)      # through a strided slice: the rest is untouched
    assert torch.equal(wide[:, 4:12], a) and bool((wide[:, :4] == 7).all()) and bool((wide[:, 12:] == 7).all())
    assert list(row_chunks(2500, STEP)) == [(0, 1000), (1000, 2000), (2000, 2500)]


def test_exact_leg_reports_swapped_rows_and_a_shifted_tile():
    X, W = small_ints((4000, 16), 1), small_ints((16, 16), 2)
    ref_fn = lambda r0, r1: X[r0:r1].double() @ W.double().t()  # noqa: E731
    H = (X.double() @ W.double().t()).float()
    assert rows_mismatch(H, ref_fn, step=STEP) is None
    assert_rows_equal(H, ref_fn, "correct", step=STEP)
    swapped = H.clone()
    swapped[[1300, 2700]] = H[[2700, 1300]]
    assert not torch.equal(swapped, H)
    msg = rows_mismatch(swapped, ref_fn, step=STEP)
    assert msg is not None and "in 2 rows" in msg and "first row 1300 (row % 256 = 20, tile % 256 = 5)" in msg and "last row 2700" in msg
    with pytest.raises(AssertionError, match="first row 1300"):
        assert_rows_equal(swapped, ref_fn, "swapped", step=STEP)
    shifted = H.clone()
    shifted[1024:1280] = H[1025:1281]                     # tile 4 reads one row too far
    msg = rows_mismatch(shifted, ref_fn, step=STEP)
    assert msg is not None and "first row 1024 (row % 256 = 0, tile % 256 = 4)" in msg
    bad = H.clone()
    bad[3999, 15] = float("nan")                          # a NaN is a difference, in the last row of the last chunk
    assert "first row 3999" in rows_mismatch(bad, ref_fn, step=STEP)


def test_exact_leg_reports_a_row_dropped_from_a_reduction():
    dH, X = small_ints((5000, 8), 5), small_ints((5000, 8), 6)
    ref = chunked_sum(lambda r0, r1: dH[r0:r1].double().t() @ X[r0:r1].double(), 5000, step=STEP)
    assert torch.equal(ref, dH.double().t() @ X.double())
    assert_small_equal(ref.float(), ref, "correct")
    row = int((dH[:, 0] * X[:, 0]).nonzero()[0])          # a row whose term in output (0, 0) is not zero
    keep = torch.ones(5000, dtype=torch.bool)
    keep[row] = False
    with pytest.raises(AssertionError, match="dropped"):
        assert_small_equal((dH[keep].double().t() @ X[keep].double()).float(), ref, "dropped")
    with pytest.raises(AssertionError):                   # the same row counted twice
        assert_small_equal((ref + dH[row:row + 1].double().t() @ X[row:row + 1].double()).float(), ref, "doubled")


def test_condition_aware_bar_is_blind_to_lost_rows_at_ten_million_rows_and_the_exact_leg_is_not():
    """Finding 1 of the large-offset work, as a fact of the suite: dW = dH^T . X over n = 1e7 rows of uniform(-1, 1) data has
    sum|term| ~ n / 4 = 2.5e6, so the bar 1e-5 * max(1, |ref|, sum|term|) is ~25 -- and a whole K-tile of 64 rows missing from the
    reduction moves an output by a random walk of 64 terms of size <= 1, far below it.  The same loss in the exact leg's integer data
    changes an integer."""
    n, f, lost = 10_000_000, 4, slice(5_000_000, 5_000_064)
    rng = np.random.default_rng(0)
    dH, X = rng.uniform(-1, 1, (n, f)), rng.uniform(-1, 1, (n, f))
    ref, absum = dH.T @ X, np.abs(dH).T @ np.abs(X)
    wrong = ref - dH[lost].T @ X[lost]
    moved = np.abs(wrong - ref).max()
    assert moved > 1.0, "the lost K-tile moves the result by far more than f32 rounding of a correct sum would"
    assert 20.0 < RTOL * absum.min() < 30.0
    assert_close(wrong, ref, "a K-tile lost, not seen", absum=absum)                       # passes: the bar's blind spot
    with pytest.raises(AssertionError):
        assert_close(wrong, ref, "a K-tile lost, seen at the GEMM bar")                    # the plain bar, which cancelling sums cannot meet
    di = rng.integers(-1, 2, (n, f)).astype(np.float32)
    xi = rng.integers(-1, 2, (n, f)).astype(np.float32)
    exact = torch.from_numpy(di.astype(np.float64).T @ xi.astype(np.float64))
    assert torch.equal(torch.from_numpy(di.T @ xi).double(), exact), "f32 arithmetic on {-1, 0, 1} data is exact"
    row = 5_000_000 + int(np.flatnonzero(di[lost, 0] * xi[lost, 0])[0])
    lost_one = exact - torch.from_numpy(np.outer(di[row], xi[row]).astype(np.float64))
    with pytest.raises(AssertionError):
        assert_small_equal(lost_one.float(), exact, "one row of 1e7 lost")


def test_rounding_leg_passes_one_ulp_and_fails_twice_the_bar():
    X = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (3000, 16)).astype(np.float32))
    W = torch.from_numpy(np.random.default_rng(2).uniform(-4, 4, (16, 16)).astype(np.float32))
    ref_fn = lambda r0, r1: X[r0:r1].double() @ W.double().t()  # noqa: E731
    H = (X.double() @ W.double().t()).float()
    assert_rows_close(H, ref_fn, "correct", step=STEP)
    ulp = H.clone()
    ulp[2100, 3] = torch.nextafter(H[2100, 3], torch.tensor(float("inf")))
    assert_rows_close(ulp, ref_fn, "one ulp", step=STEP)
    assert rows_mismatch(ulp, ref_fn, step=STEP) is not None, "the exact leg sees one ulp"
    off = H.clone()
    off[2100, 3] += 2e-5 * max(1.0, abs(float(H[2100, 3])))
    with pytest.raises(AssertionError, match="first row 2100"):
        assert_rows_close(off, ref_fn, "2e-5 off", step=STEP)
    with pytest.raises(AssertionError):
        assert_close(off.numpy(), H.numpy(), "2e-5 off")
    assert_close(ulp.numpy(), H.numpy(), "one ulp")
    # the absolute and the whole-matrix-scale forms, and the mask of elements that count
    with pytest.raises(AssertionError):
        assert_rows_close(off, ref_fn, "atol", atol=1e-6, step=STEP)
    assert_rows_close(ulp, ref_fn, "atol", atol=1e-5, step=STEP)
    with pytest.raises(AssertionError):
        assert_rows_close(off, ref_fn, "scale", rtol=1e-6, ref_scale=1.0, step=STEP)
    masked = lambda r0, r1: (ref_fn(r0, r1), torch.ones((r1 - r0, 16), dtype=torch.bool).index_fill_(1, torch.tensor([3]), False))  # noqa: E731
    assert_rows_close(off, masked, "column 3 does not count", step=STEP)
    with pytest.raises(AssertionError):
        assert_rows_close(off, lambda r0, r1: (ref_fn(r0, r1), torch.ones((r1 - r0, 16), dtype=torch.bool)), "counts", step=STEP)


def test_gathered_rows_helper_reports_a_wrong_slot():
    env = dict(torch=torch)
    X = small_ints((2_500_000, 2), 9)                    # three reference chunks
    idx = torch.tensor([5, 2_400_000, 1_000_000, 5, 999_999, 0], dtype=torch.int32)
    got = X[idx.long()]
    src_fn = lambda r0, r1: X[r0:r1].double()  # noqa: E731
    big.assert_gathered_equal(env, got, idx, src_fn, X.shape[0], "correct")
    bad = got.clone()
    bad[2] = X[1_000_001] + 5.0                          # the neighbouring row, made surely different
    with pytest.raises(AssertionError, match="first slot 2 <- row 1000000"):
        big.assert_gathered_equal(env, bad, idx, src_fn, X.shape[0], "wrong slot")
    assert big.first_argmax(torch, torch.tensor([[1.0, 3.0, 3.0], [2.0, 0.0, 2.0]])).tolist() == [1, 0]


def test_row_sample_and_tile_plan_facts():
    """The sampled rows are the ones the issue names, and the three row counts of leg A have the tile-plan facts they were chosen for."""
    M = 10_000_000
    rows = sample_rows(M)
    assert np.array_equal(rows, np.unique(rows)) and rows[0] == 0 and rows[-1] == M - 1
    have = set(rows.tolist())
    assert set(range(600)) <= have and set(range(8_388_300, 8_388_901)) <= have and set(range(M - 700, M)) <= have
    assert {256_000, 256_255, 39 * 256_000, 39 * 256_000 + 255} <= have
    last_round = range((39062 - 150 - 256) * 256, (39062 - 150) * 256)
    assert set(last_round) <= have and rows.size >= 600 + 601 + 80 + 65536 + 700 + 2900
    assert np.array_equal(sample_rows(M), rows) and sample_rows(5000).max() == 4999
    assert [dma_tail_round(m) for m in big.ROW_COUNTS] == [150, 100, 40]
    for m in big.ROW_COUNTS:
        big.check_plan(m)
    T = torch.arange(30, dtype=torch.float32).reshape(10, 3)
    assert np.array_equal(take_rows(T, np.array([0, 4, 9]), step=4), T[[0, 4, 9]].numpy())
