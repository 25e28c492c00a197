"""CPU tests of tests/gemm_fused_ref.py, what tests/test_gpu_gemm_fused.py holds the fused transform epilogues to: every case's
integer operands meet the exactness condition (no case exempt); the restated launch plan, run over the case table, reaches every
geometry, tail length, multi-tile walk and decline; the references agree with plain Python loops; and the comparisons of the GPU
file reject deliberately wrong restatements of the kernels on the table's own inputs."""
import numpy as np
import pytest

from tests import gemm_fused_ref as R
from tests.elementwise_ref import BF16_TABLE, bf16_rne_ref

F32 = np.float32
ALL_SHAPES = sorted({(c.M, c.N, c.K) for c in R.RELU_CASES + R.BN_CASES})


# ---------------------------------------------------------------------------------------------- exactness, every case
@pytest.mark.parametrize("M,N,K", ALL_SHAPES, ids=lambda v: str(v))
def test_every_case_meets_the_exactness_condition(M, N, K):
    """relu_data and bn_data assert the condition themselves (and the GPU file calls them before any GPU call); here it is checked
    once more, spelled out, for every shape of both tables: integers, sum|C| < 2^24 on all three exact legs, sum|d| and sum d^2
    < 2^24 with d = H - H[0]."""
    for leg, d in R.relu_data(M, N, K).items():
        C = d["C"].astype(np.float64)
        assert np.array_equal(C, np.rint(C)) and np.abs(C).sum(0).max() < 2.0 ** 24, leg
        assert np.array_equal(d["colsum"], C.sum(0))
    b = R.bn_data(M, N, K)
    dd = b["H"] - b["H"][0]
    assert np.array_equal(dd, np.rint(dd)) and np.abs(dd).sum(0).max() < 2.0 ** 24 and (dd * dd).sum(0).max() < 2.0 ** 24
    m2, v2 = R.bn_stats_ref(b["H"])                           # the two-pass float64 statistics agree with the one-rounding form
    assert np.allclose(b["mean"], m2, rtol=1e-12, atol=1e-12) and np.allclose(b["var"], v2, rtol=1e-11, atol=1e-12)


def test_the_tall_cases_need_the_sparse_operands():
    """What the density switch is for: at P(nonzero) = 2 / 3 the tallest 512-wide case breaks sum d^2 < 2^24 (so the assertion,
    not a figure in a comment, decides)."""
    M, N, K = 256 * 130 + 1, 512, 128
    X, W = R.int_matrix(M, K, 1), R.int_matrix(N, K, 2)
    with pytest.raises(AssertionError):
        R.bn_exact_stats(X.astype(np.float64) @ W.astype(np.float64).T)


# ---------------------------------------------------------------------------------------------- coverage of the table
def test_the_table_reaches_every_cell():
    relu = {c.name: R.plan(c.M, c.N, c.K, R.relu_aligned(c)) for c in R.RELU_CASES}
    bn = {c.name: R.plan(c.M, c.N, c.K, R.bn_aligned(c)) for c in R.BN_CASES}
    for plans in (relu, bn):
        fused = [p for p in plans.values() if p.rows]
        assert {p.geometry for p in fused} == {"256x256", "256x128", "NG"}
        for geo in ("256x256", "256x128", "NG"):
            assert {p.tail for p in fused if p.geometry == geo} >= ({0, 255, 1} if geo == "256x256" else {255}), geo
            assert any(p.m_tiles > p.gy for p in fused if p.geometry == geo), f"{geo}: no workgroup walks more than one M-tile"
            assert any(p.m_tiles == p.gy for p in fused if p.geometry == geo)
        assert {(p.gy, p.m_tiles) for p in fused if p.m_tiles > p.gy} == {(86, 87), (128, 130), (256, 257)}
        assert {p.decline for p in plans.values() if not p.rows} == {"K % 64", "N % 4", "N < 64", "M < 2048", "off the 16-byte grid"}
    assert R.plan(R.RELU_EMPTY.M, R.RELU_EMPTY.N, R.RELU_EMPTY.K).decline == "M == 0"
    # every operand in turn off the grid; W off the grid leaves the BatchNorm product fused
    for M, N, K in R.LAYOUT_SHAPES:
        for lay in ("oaaa", "aoaa", "aaoa", "aaao"):
            assert relu[f"{M}x{N}x{K}-{lay}"].rows == 0 and relu[f"{M}x{N}x{K}"].rows == 2048
            assert bn[f"{M}x{N}x{K}-{lay}"].rows == (2048 if lay == "aoaa" else 0)
    # guarded tile: a column group wholly off (N = 64), a last tile of 4 columns (N = 132), widths below and above one tile
    ng = {c.N for c in R.RELU_CASES if relu[c.name].geometry == "NG"}
    assert ng == {64, 68, 100, 132, 192, 252}
    assert {c.K for c in R.RELU_CASES if relu[c.name].geometry == "NG"} == {64, 128, 192}
    assert {c.K for c in R.RELU_CASES if relu[c.name].geometry == "256x256"} == {64, 128, 192}
    # siblings: the bf16 entry on a whole tile, the guarded tile and a ragged tail; the slot pack fused at N % 128 == 0 only
    assert [R.fused_rows_bf16(*s) for s in R.BF16_SHAPES] == [2048, 2048, 2048] and R.plan(*R.BF16_SHAPES[1]).geometry == "NG"
    assert R.fused_rows_bf16(2047, 256, 64) is None and R.fused_rows_bf16(2303, 256, 64, aligned=False) is None
    assert [R.fused_rows_slots(*s) for s in R.SLOT_SHAPES] == [2303, 2303, 0]
    assert R.fused_rows(2303, 256, 64) == 2048 and R.fused_rows(2047, 256, 64) == 0 and R.fused_rows(2303, 256, 64, aligned=False) == 0


def test_mask_values_fill_tiles_and_tail():
    """Rows of every value, and rows that mix all of them, inside a fused tile and inside the 255-row tail of M = 2303."""
    Y = R.mask_values_y(2303, 100)
    for rows in (slice(256, 512), slice(2048, 2303)):
        blk = Y[rows]
        for v in R.MASK_VALUES:
            same = (blk.view(np.int32) == np.array([v], dtype=F32).view(np.int32)).all(1)
            assert same.any(), f"no whole row of {v!r}"
        assert (np.array([len(set(r.view(np.int32).tolist())) for r in blk]) == 10).any()
    keep = R.MASK_VALUES > 0
    assert keep.tolist() == [False, False, True, False, True, False, True, False, True, False]


# ---------------------------------------------------------------------------------------------- references against plain loops
def test_references_agree_with_plain_loops():
    M, N, K = 70, 12, 8
    A, B = R.int_matrix(M, K, 11), R.int_matrix(K, N, 12)
    Y = R.mask_values_y(M, N)
    C, colsum = R.relu_colsum_ref(A, B, Y)
    for m in range(M):
        for n in range(N):
            acc = 0.0
            for k in range(K):
                acc += float(A[m, k]) * float(B[k, n])
            y = float(Y[m, n])
            want = acc if y > 0 else 0.0                     # Python's > is IEEE: NaN and -0.0 drop
            assert C[m, n] == want and (want != 0 or not np.signbit(C[m, n]))
    assert np.array_equal(colsum, [sum(C[m, n] for m in range(M)) for n in range(N)])
    H = A.astype(np.float64) @ B.astype(np.float64)
    mean, var = R.bn_stats_ref(H)
    em, ev, _ = R.bn_exact_stats(H)
    for n in range(N):
        mu = sum(H[m, n] for m in range(M)) / M
        v = sum((H[m, n] - mu) ** 2 for m in range(M)) / M
        assert abs(mean[n] - mu) <= 1e-13 and abs(var[n] - v) <= 1e-12 and abs(em[n] - mu) <= 1e-13 and abs(ev[n] - v) <= 1e-12
    # bf16: the table's expected patterns against torch's own conversion
    import torch
    finite = R.BF16_FINITE
    want = torch.from_numpy(finite.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bf16_rne_ref(finite), want) and len(finite) == len(BF16_TABLE) - 2


# ---------------------------------------------------------------------------------------------- the comparisons can fail
def rejected(fn, *args):
    try:
        fn(*args, "wrong restatement")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("M,N,K", [(2303, 256, 64), (2303, 100, 64), (256 * 87 + 9, 384, 64)], ids=lambda v: str(v))
def test_wrong_masks_and_wrong_sums_are_rejected(M, N, K):
    data = R.relu_data(M, N, K)
    rows = R.fused_rows(M, N, K)

    def product(d):
        with np.errstate(all="ignore"):
            return (d["A"].astype(np.float64) @ d["B"].astype(np.float64)).astype(F32)      # float32: 2^127 * 2 overflows as on the device

    def run(d, mask):
        with np.errstate(all="ignore"):
            C = mask(product(d), d["Y"])
            return C, C.astype(np.float64).sum(0)

    select = lambda P, Y: np.where(Y > 0, P, F32(0))                                   # noqa: E731
    wrong = {
        "mask by >= 0": ("exact", lambda P, Y: np.where(Y >= 0, P, F32(0))),
        "mask by multiplication": ("exact", lambda P, Y: P * (Y > 0).astype(F32)),
        "mask by multiplication, infinite products": ("poison", lambda P, Y: P * (Y > 0).astype(F32)),
        "NaN kept": ("mask", lambda P, Y: np.where(~(Y <= 0), P, F32(0))),
        "denormal flushed": ("mask", lambda P, Y: np.where(np.where(np.abs(Y) < R.FLT_MIN, F32(0), Y) > 0, P, F32(0))),
    }
    for leg in data:                                                                   # the right restatement passes every leg
        C, colsum = run(data[leg], select)
        R.check_relu_colsum(C, colsum, data[leg], leg)
    for what, (leg, mask) in wrong.items():
        C, colsum = run(data[leg], mask)
        assert rejected(R.check_relu_colsum, C, colsum, data[leg]), what
        good = run(data[leg], select)[0]
        if "multiplication" not in what:      # the sums alone notice it too (a product with -0 for +0 has the same sums)
            assert rejected(R.check_relu_colsum, good, colsum, data[leg]), what + " (sums)"
    for leg in ("exact", "mask", "poison"):
        d = data[leg]
        C = d["C"]
        sums = {"without the tail rows": C[:rows].astype(np.float64).sum(0),
                "one M-tile counted twice": d["colsum"] + C[256:512].astype(np.float64).sum(0),
                "the last M-tile of a workgroup's walk dropped": d["colsum"] - C[rows - 256:rows].astype(np.float64).sum(0)}
        if N % 128:
            s = d["colsum"].copy()
            s[N // 128 * 128:] = 0
            sums["without the last tile's columns"] = s
        for what, s in sums.items():
            assert rejected(R.check_relu_colsum, C, s, d), f"{leg}: {what}"


@pytest.mark.parametrize("M,N,K", [(2303, 256, 64), (2303, 100, 64), (256 * 257 + 3, 100, 64)], ids=lambda v: str(v))
def test_wrong_batchnorm_sums_are_rejected(M, N, K):
    b = R.bn_data(M, N, K)
    H, rows = b["H"], R.fused_rows(M, N, K)
    R.check_bn_fused(b["mean"].astype(F32), b["var"].astype(F32), b, "the right statistics")
    d = H - H[0]

    def finish(S, Q):
        m = S / M
        return (H[0] + m).astype(F32), np.maximum(Q / M - m * m, 0.0).astype(F32)

    S, Q = d.sum(0), (d * d).sum(0)
    R.check_bn_fused(*finish(S, Q), b, "the kernel's formula")
    wrong = {"without the tail rows": finish(d[:rows].sum(0), (d[:rows] ** 2).sum(0)),
             "one M-tile counted twice": finish(S + d[256:512].sum(0), Q + (d[256:512] ** 2).sum(0)),
             "squares of one M-tile dropped": finish(S, Q - (d[256:512] ** 2).sum(0)),
             "unbiased variance": (finish(S, Q)[0], (finish(S, Q)[1].astype(np.float64) * M / (M - 1)).astype(F32))}
    for what, (mean, var) in wrong.items():
        assert rejected(R.check_bn_fused, mean, var, b), what


@pytest.mark.parametrize("M,N,K,offset", R.OFFSET_CASES, ids=lambda v: str(v))
def test_unshifted_float32_variance_is_rejected_by_the_offset_bar(M, N, K, offset):
    """E[h^2] - E[h]^2 with float32 sums and no shift -- what the epilogue's shift by row 0 is there to avoid -- misses the offset
    leg's bar; the shifted sums finished in double pass it."""
    X, W = R.offset_operands(M, N, K, offset)
    H = (X.astype(np.float64) @ W.astype(np.float64).T).astype(F32)
    d = H - H[0]
    S, Q = d.sum(0, dtype=np.float64), (d.astype(np.float64) ** 2).sum(0)
    rtol = R.offset_var_rtol(M, N, K, offset)
    assert 0 < rtol <= 1e-4
    R.check_bn_offset((H[0] + S / M).astype(F32), (Q / M - (S / M) ** 2).astype(F32), H, rtol, "shifted")
    s = q = np.zeros(N, dtype=F32)
    for m in range(M):                                       # float32 running sums, row by row
        s = s + H[m]
        q = q + H[m] * H[m]
    mean = s / F32(M)
    var = q / F32(M) - mean * mean
    assert rejected(R.check_bn_offset, mean, var, H, rtol)
    assert rejected(R.check_bn_offset, mean, var, H, 1e-4), "even the bar of tests/test_gpu_parity.py rejects it"


def test_bf16_by_truncation_is_rejected():
    for M, N, K in R.BF16_SHAPES:
        ref = R.bf16_data(M, N, K)
        u = ref["H"].view(np.uint32)
        good = bf16_rne_ref(np.where(np.isnan(ref["H"]), np.uint32(0x7FC00000), u))
        R.check_bf16(good, ref, "round to nearest even")
        assert rejected(R.check_bf16, (u >> 16).astype(np.uint16), ref)
        flushed = good.copy()                                 # a NaN column that came out as +-0 or inf
        flushed[:, ref["nan_col"]] = 0x7F80
        assert rejected(R.check_bf16, flushed, ref)
        # every special value passes through whole tiles and through the ragged tail, in every column
        for rows in (slice(0, 2048), slice(2048, M)):
            assert {int(v) for v in np.unique(u[rows][:, ref["keep"]])} == {int(v) for v in R.BF16_FINITE if v != 0x80000000}
