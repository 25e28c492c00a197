"""References, comparisons and the case table of the fused transform epilogues of gemm_dma_kernel (gnn.cpp_amd/csrc/gnnx_gemm.hip):
gnnx_gemm_relu_colsum_f32, gnnx_gemm_bn_stats_f32, gnnx_gemm_nt_bf16out_f32 and gnnx_gemm_nt_rows_to_slots_f32
(tests/test_gpu_gemm_fused.py runs them; tests/test_gemm_fused_ref_cpu.py proves the table's coverage and that the comparisons can fail).

The references are plain float64 NumPy and restate no summation order.  The sums are made order-free by the data: operands come
from {-1, 0, 1}, every product entry is an integer, and per column

    sum_m |C[m][n]| < 2^24                                     (ReLU-colsum: `relu_data`)
    sum_m |d| < 2^24 and sum_m d^2 < 2^24,  d = H - H[0]       (BatchNorm sums: `bn_data`; H[0] is the kernel's shift)

are ASSERTED on every case before anything is compared.  Every partial sum of any subset in any order is then an integer below
2^24, which float32 holds exactly: the float32 sums have one right value and the comparison is equality (column sums), one
float32 ulp (the mean: S exact, finished in double, one cast) and 2^-23 var + 2^-50 Q / M (the variance: Q exact, the double
arithmetic of Q / M - (S / M)^2 errs by a few 2^-53 Q / M, one cast).

`plan` restates launch_dma / launch_dma_geo for the four epilogues: which geometry a shape runs on, how many leading rows the
fused kernel takes, how many M-tiles a workgroup walks, and why a call is declined.  It proves coverage; it is never a second
implementation of the arithmetic."""
import functools
from collections import namedtuple

import numpy as np

from tests.elementwise_ref import BF16_TABLE, bf16_rne_ref, rows_to_slots_ref, send_list, slot_table_ref
from tests.gemm_ref import dma_shape_ok
from tests.helpers import NUM_CU, RTOL, fill_small_ints
from tests.norm_ref import assert_bits, bits, check_exact, f32

TILE = 256
FLT_MIN = np.float32(2.0 ** -126)

# ---------------------------------------------------------------------------------------------- the case table
# layout: one letter per operand, "a" = helpers.embed(..., "a") (on the 16-byte grid, pitch a multiple of 4 and wider than the row),
# "o" = odd pitch and a base off the grid.  ReLU-colsum: A, B, C, Y.  BatchNorm: X, W, H and the workspace ("a", or "o" = the
# pointer moved up by 4 bytes).
Case = namedtuple("Case", "name M N K layout kind")

GEOMETRY_SHAPES = ([(2048, 256, 64), (2303, 256, 64), (2305, 256, 64), (2303, 512, 64), (2303, 128, 64), (2303, 384, 64)] +
                   [(2303, N, 64) for N in (64, 68, 100, 132, 192, 252)] +
                   [(2303, N, K) for K in (128, 192) for N in (256, 100)])
MULTI_TILE_SHAPES = [(256 * 87 + 9, 384, 64), (256 * 130 + 1, 512, 64), (256 * 257 + 3, 256, 64), (256 * 257 + 3, 100, 64)]
FALLBACK_SHAPES = [(2047, 256, 64), (2303, 256, 96), (2303, 130, 64), (2303, 60, 64), (1, 256, 64)]
LAYOUT_SHAPES = [(2303, 256, 64), (2303, 100, 64)]


def _cases(base, variants):
    out = [Case(f"{M}x{N}x{K}", M, N, K, base, kind) for kind, shapes in (("geometry", GEOMETRY_SHAPES), ("multi-tile", MULTI_TILE_SHAPES),
                                                                           ("fallback", FALLBACK_SHAPES)) for M, N, K in shapes]
    out += [Case(f"{M}x{N}x{K}-{lay}", M, N, K, lay, "layout") for M, N, K in LAYOUT_SHAPES for lay in variants]
    return out


RELU_CASES = _cases("aaaa", ("oaaa", "aoaa", "aaoa", "aaao"))
RELU_EMPTY = Case("0x256x64", 0, 256, 64, "aaaa", "empty")           # GNNX_OK and colsum == 0: no other leg applies
BN_CASES = _cases("aaaa", ("oaaa", "aoaa", "aaoa", "aaao"))
OFFSET_CASES = [(M, N, K, off) for M, N, K in LAYOUT_SHAPES for off in (3.0, -20.0)]
BF16_SHAPES = [(2303, 256, 64), (2303, 100, 64), (2303, 128, 128)]
SLOT_SHAPES = [(2303, 128, 64), (2303, 256, 64), (2303, 64, 64)]
SLOT_PER_ROW = (0, 1, 7, 2)
SLOT_SPARE = 3                                                        # rows of `send` that no list names: they keep the sentinel

# tests/test_gpu_gemm_fused.py::test_bn_stats_offset_leg: the largest relative variance error measured on an MI355X per offset case
# (README, test section; the 100-wide W is the first 100 rows of the 256-wide one and holds its worst column), and the bar: 8 x that
# figure, never above the 1e-4 of tests/test_gpu_parity.py.  The margin covers a different rounding of `shift` (row 0 of H) from
# another compiler, nothing more.
OFFSET_VAR_MEASURED = {(2303, 256, 64, 3.0): 7.186e-07, (2303, 256, 64, -20.0): 7.095e-07, (2303, 100, 64, 3.0): 7.186e-07,
                       (2303, 100, 64, -20.0): 7.095e-07}


def offset_var_rtol(M, N, K, offset):
    return min(1e-4, 8.0 * OFFSET_VAR_MEASURED[(M, N, K, offset)])


def case_id(c):
    return c.name


# ---------------------------------------------------------------------------------------------- launch_dma, restated
Plan = namedtuple("Plan", "rows geometry m_tiles gy tail decline")


def decline_reason(M, N, K, aligned=True):
    """Why launch_dma takes no row of a column-sum product (None: it takes some), in the order the code asks."""
    if M == 0:
        return "M == 0"
    if K % 64:
        return "K % 64"
    if N % 4:
        return "N % 4"
    if N < 64:
        return "N < 64"
    if M < 8 * TILE:
        return "M < 2048"
    if not aligned:
        return "off the 16-byte grid"
    return None


def plan(M, N, K, aligned=True):
    """launch_dma<kReluColsum / kBnSums>: floor(M / 256) whole tiles on 256 x 256 (N % 256 == 0), 256 x 128 (N % 128 == 0) or the
    guarded 256 x 128 tile (NG); one workgroup per CU, gy = ceil(256 / column tiles) workgroups per column, each walking
    ceil(m_tiles / gy) M-tiles."""
    why = decline_reason(M, N, K, aligned)
    assert (why is None) == (dma_shape_ok(M, N, K) and aligned)
    if why:
        return Plan(0, None, 0, 0, M, why)
    geometry, bn = ("256x256", 256) if N % 256 == 0 else ("256x128", 128) if N % 128 == 0 else ("NG", 128)
    m_tiles, cols = M // TILE, -(-N // bn)
    gy = min(-(-NUM_CU // cols), m_tiles)
    return Plan(m_tiles * TILE, geometry, m_tiles, gy, M - m_tiles * TILE, None)


def fused_rows(M, N, K, aligned=True):
    """Leading rows the fused kernel takes for a column-sum epilogue (gnnx_gemm_relu_colsum_f32, gnnx_gemm_bn_stats_f32)."""
    return plan(M, N, K, aligned).rows


def fused_rows_bf16(M, N, K, aligned=True):
    """gnnx_gemm_nt_bf16out_f32: whole tiles by the kernel, the ragged rows by product + rounding; None: GNNX_ERR_SHAPE."""
    return M // TILE * TILE if dma_shape_ok(M, N, K) and aligned else None


def fused_rows_slots(M, N, K, aligned=True):
    """gnnx_gemm_nt_rows_to_slots_f32: the kernel has no guarded column tile (N % 128 == 0) and covers ragged rows by one more,
    overlapping tile; everything else is the two-call path."""
    return M if dma_shape_ok(M, N, K) and N % 128 == 0 and aligned else 0


def relu_aligned(case):
    return case.layout == "aaaa"


def bn_aligned(case):
    """W is read by the scalar transpose only: its layout does not matter."""
    return case.layout[0] == "a" and case.layout[2] == "a" and case.layout[3] == "a"


# ---------------------------------------------------------------------------------------------- integer operands
def tall(M):
    return M >= 3000


def int_matrix(rows, cols, seed, sparse=False):
    """[rows, cols] float32 of {-1, 0, 1}: uniform (P(nonzero) = 2 / 3), or sparse (P(-1) = P(1) = 1 / 8) for the tall cases."""
    import torch
    gen = torch.Generator()
    gen.manual_seed(int(seed))
    t = torch.empty((rows, cols), dtype=torch.float32)
    if not t.numel():
        return t.numpy()
    if not sparse:
        return fill_small_ints(t, gen).numpy()
    fill_small_ints(t, gen, 0, 7)
    return ((t == 1).float() - (t == 0).float()).numpy()


def mask_matrix(rows, cols, seed):
    """Y of the exact leg: {-1, 0, 1} with half of the entries kept (P(1) = 1 / 2, P(0) = P(-1) = 1 / 4)."""
    import torch
    gen = torch.Generator()
    gen.manual_seed(int(seed))
    t = fill_small_ints(torch.empty((rows, cols), dtype=torch.float32), gen, 0, 3)
    return torch.where(t >= 2, torch.ones_like(t), t - 1).numpy()


def _seed(M, N, K, salt):
    return (M * 1_000_003 + N * 1009 + K * 17 + salt) % (1 << 31)


def relu_colsum_ref(A, B, Y):
    """(C, colsum) in float64: C = where(Y > 0, A64 @ B64, +0) with IEEE `>` -- a positive denormal and +inf keep the entry; -0, +0,
    NaN and -inf drop it; a dropped position is +0 whatever the product is."""
    with np.errstate(all="ignore"):
        P = np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64)
        C = np.where(f32(Y) > 0, P, 0.0)
    return C, C.sum(0)


def assert_colsum_exact(C64):
    """The exactness condition of the ReLU-colsum sums: integers, and sum_m |C[m][n]| < 2^24 in every column."""
    check_exact(np.abs(C64), 1.0)


MASK_VALUES = np.array([0.0, -0.0, 1e-45, -1e-45, FLT_MIN, np.nan, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32)


def mask_values_y(M, N):
    """Y of the mask-values leg.  Blocks of ten rows alternate between whole rows of one value (row m holds MASK_VALUES[m % 10]) and
    rows that walk through all of them (column n holds MASK_VALUES[(m + n) % 10]): every value fills whole rows, and every 16-byte
    group of a lane mixes kept and dropped entries, inside every 256-row tile and inside a 255-row tail."""
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    return MASK_VALUES[(m + n * ((m // 10) % 2)) % 10]


def poisoned_rows(M):
    """One row inside the second tile and the last row (inside the ragged tail where there is one)."""
    return sorted({min(300, M - 1), M - 1})


def poison(A, B, Y):
    """The poisoned-products leg: B entries of +-2, 2^127 all along a few rows of A (their products are +-inf, and inf - inf = NaN
    where a column of B mixes signs), Y <= 0 on the whole of those rows."""
    A, B, Y = A.copy(), B * np.float32(2), Y.copy()
    for r in poisoned_rows(A.shape[0]):
        A[r, :] = np.float32(2.0 ** 127)
        Y[r, :] = -(np.arange(Y.shape[1]) % 2).astype(np.float32)
    return A, B, Y


@functools.lru_cache(maxsize=2)
def relu_data(M, N, K):
    """Integer operands of a ReLU-colsum case and the float64 references of its three exact legs, exactness asserted."""
    A, B = int_matrix(M, K, _seed(M, N, K, 1), tall(M)), int_matrix(K, N, _seed(M, N, K, 2), tall(M))
    Y = mask_matrix(M, N, _seed(M, N, K, 3))
    legs = {"exact": (A, B, Y), "mask": (A, B, mask_values_y(M, N)), "poison": poison(A, B, Y)}
    out = {}
    for leg, (a, b, y) in legs.items():
        C, colsum = relu_colsum_ref(a, b, y)
        assert_colsum_exact(C)
        out[leg] = dict(A=a, B=b, Y=y, C=C.astype(np.float32), colsum=colsum)        # C: integers below 2^24, exact in float32
    return out


def check_relu_colsum(C, colsum, ref, what):
    """The comparison of the three exact legs: C bit for bit, the column sums EQUAL to the float64 sums."""
    assert_bits(C, ref["C"], f"{what}: C")
    got = np.asarray(colsum, dtype=np.float64)
    bad = ~(got == ref["colsum"])                                     # a NaN differs
    assert not bad.any(), (f"{what}: colsum differs from the float64 sums in {int(bad.sum())} of {bad.size} columns, first {int(np.argmax(bad))}: "
                           f"got {got[np.argmax(bad)]!r}, expected {ref['colsum'][np.argmax(bad)]!r}")


def check_colsum_rounding(colsum, C, what):
    """The rounding leg: |colsum - float64 sum| <= 1e-5 * max(1, sum_m |C|) per column."""
    C64 = np.asarray(C, dtype=np.float64)
    err, bound = np.abs(np.asarray(colsum, dtype=np.float64) - C64.sum(0)), RTOL * np.maximum(1.0, np.abs(C64).sum(0))
    assert (err <= bound).all(), f"{what}: colsum err / bound = {float((err / bound).max()):.3f}"


# ---------------------------------------------------------------------------------------------- BatchNorm statistics
def bn_stats_ref(H64):
    """Column mean and biased variance in float64, two passes."""
    H64 = np.asarray(H64, dtype=np.float64)
    mean = H64.mean(0)
    return mean, ((H64 - mean) ** 2).mean(0)


def bn_exact_stats(H64):
    """(mean, var, Q) of an integer H with the condition asserted: S = sum d and Q = sum d^2, d = H - H[0], are exact integers, so
    mean = H[0] + S / M and var = (M Q - S^2) / M^2 carry ONE float64 rounding each (M Q and S^2 stay below 2^53)."""
    H64 = np.asarray(H64, dtype=np.float64)
    M = H64.shape[0]
    d = H64 - H64[0]
    check_exact(d, 1.0)
    check_exact(d * d, 1.0)
    S, Q = d.sum(0), (d * d).sum(0)
    assert (M * Q < 2.0 ** 53).all() and (S * S < 2.0 ** 53).all()
    return H64[0] + S / M, (M * Q - S * S) / (float(M) * M), Q


@functools.lru_cache(maxsize=2)
def bn_data(M, N, K):
    """Integer X [M, K] and W [N, K] (row N // 3 of W all zero: a column of H with variance exactly 0), H = X . W^T in float64 and
    its exact statistics."""
    X, W = int_matrix(M, K, _seed(M, N, K, 4), tall(M)), int_matrix(N, K, _seed(M, N, K, 5), tall(M))
    W[N // 3] = 0
    H = X.astype(np.float64) @ W.astype(np.float64).T
    mean, var, Q = bn_exact_stats(H)
    assert var[N // 3] == 0.0
    return dict(X=X, W=W, H=H, mean=mean, var=var, Q=Q)


def check_bn_fused(mean, var, ref, what):
    """Where the fused kernel ran: mean within one float32 ulp of the float64 mean; var within 2^-23 var64 + 2^-50 Q / M, and
    exactly 0 where var64 is 0 (Q / M - (S / M)^2 is then an exact 0 or a rounding residue the clamp and the bound both allow: the
    zero column of W has Q = 0)."""
    M = ref["H"].shape[0]
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ulp = np.spacing(np.abs(ref["mean"]).astype(np.float32)).astype(np.float64)
    err = np.abs(mean - ref["mean"])
    assert (err <= ulp).all(), f"{what}: mean off by {float((err / ulp).max()):.2f} ulp in column {int(np.argmax(err / ulp))}"
    err, bound = np.abs(var - ref["var"]), 2.0 ** -23 * ref["var"] + 2.0 ** -50 * ref["Q"] / M
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: var outside 2^-23 var + 2^-50 Q / M in {int(bad.sum())} columns, first {int(np.argmax(bad))}: got "
                           f"{var[np.argmax(bad)]!r}, expected {ref['var'][np.argmax(bad)]!r}")


def offset_operands(M, N, K, offset):
    """Uniform X + offset and W of the offset leg (the package's portable generator: the same values on the host and on the device)."""
    from tests.helpers import synth
    return synth.uniform_pm1(85, (M, K)) + np.float32(offset), synth.uniform_pm1(86, (N, K), scale=K ** -0.5)


def offset_errors(mean, var, H):
    """(mean error over its bar 1e-5 * max(1, max|mean64|), largest relative variance error) against float64 on the same H."""
    m64, v64 = bn_stats_ref(H)
    return (float(np.abs(np.asarray(mean, dtype=np.float64) - m64).max() / (RTOL * max(1.0, float(np.abs(m64).max())))),
            float((np.abs(np.asarray(var, dtype=np.float64) - v64) / np.maximum(v64, 1e-30)).max()))


def check_bn_offset(mean, var, H, rtol, what):
    em, ev = offset_errors(mean, var, H)
    assert em <= 1.0, f"{what}: mean err / bound = {em:.3f}"
    assert ev <= rtol, f"{what}: relative variance error {ev:.3e} > {rtol:.3e}"


# ---------------------------------------------------------------------------------------------- bf16 output
BF16_FINITE = BF16_TABLE[np.isfinite(BF16_TABLE.view(np.float32))]


def bf16_data(M, N, K):
    """One-hot X (row m holds a single 1 at column m % K) and W = the finite patterns of BF16_TABLE tiled over [N, K]: every other
    term of H[m][n] is an exact zero, so H[m][n] is W[n][m % K] in any order -- with one exception the data cannot avoid: where
    W holds -0 the sum of that -0 and the +-0 of the other terms is +0 (the accumulators start at +0).  A -0 OUTPUT still passes
    through the cast: the negative denormals round to it.  Row N - 2 of W holds one NaN: that column of H is NaN."""
    X = np.zeros((M, K), dtype=np.float32)
    X[np.arange(M), np.arange(M) % K] = 1
    W = BF16_FINITE[np.arange(N * K) % len(BF16_FINITE)].reshape(N, K).view(np.float32).copy()
    nan_col = N - 2
    W[nan_col, 3] = np.nan
    with np.errstate(all="ignore"):
        H = (X.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    want = W[:, np.arange(M) % K].T
    keep = np.ones(N, dtype=bool)
    keep[nan_col] = False
    minus0 = bits(want) == np.int32(-2 ** 31)
    assert np.isnan(H[:, nan_col]).all() and (bits(H) == np.where(minus0, 0, bits(want)))[:, keep].all()
    expected = bf16_rne_ref(H[:, keep].view(np.uint32))
    return dict(X=X, W=W, H=H, nan_col=nan_col, keep=keep, expected=expected)


def check_bf16(got_u16, ref, what):
    """Bit patterns equal to the round-to-nearest-even reference; the NaN column is NaN (exponent all ones, a non-zero mantissa)."""
    got_u16 = np.asarray(got_u16).view(np.uint16)
    col = got_u16[:, ref["nan_col"]]
    assert ((col & 0x7F80) == 0x7F80).all() and ((col & 0x007F) != 0).all(), f"{what}: the NaN column is not NaN in bf16"
    bad = got_u16[:, ref["keep"]] != ref["expected"]
    if bad.any():
        r, c = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bf16 patterns differ, first at row {r}: got "
                             f"{int(got_u16[:, ref['keep']][r, c]):#06x}, expected {int(ref['expected'][r, c]):#06x} "
                             f"for float32 {int(ref['H'][:, ref['keep']].view(np.uint32)[r, c]):#010x}")


# ---------------------------------------------------------------------------------------------- slot pack
def slot_data(M, N, K, sentinel):
    X, W = int_matrix(M, K, _seed(M, N, K, 6)), int_matrix(N, K, _seed(M, N, K, 7))
    H = X.astype(np.float64) @ W.astype(np.float64).T
    idx = send_list(M, SLOT_PER_ROW)
    table = slot_table_ref(idx, M)
    n_slots = len(idx) + SLOT_SPARE
    return dict(X=X, W=W, H=H, table=table, n_slots=n_slots, send=rows_to_slots_ref(H.astype(np.float32), table, n_slots, sentinel))

