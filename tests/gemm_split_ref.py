"""NumPy reference of the opt-in split-precision product gnnx_gemm_split_bf16_f32 (gnn.cpp_amd/csrc/gnnx_gemm_split.hip), pinned by
tests/test_gemm_split_ref_cpu.py and used by tests/test_gpu_gemm_split.py.  It restates the CONTRACT of include/gnnx.h, not the kernel:

  bf16_rne / split3   the header's split  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), subtractions in float32;
  kept_terms64        the float64 sum of the six piece products with i + j <= 2;  absum  |A| . |B|^T in float64;
  exact families      integer operands on which the device result must EQUAL the int64 product A . B^T whatever the order of the
                      additions and however a matrix instruction rounds inside, because nothing is ever rounded:

      family   A                       B                       piece products that carry the result
      A3B1     integers, |a| < 2^19    {-1, 0, 1}              a0.b0  a1.b0  a2.b0
      A1B3     {-1, 0, 1}              integers, |b| < 2^19    a0.b0  a0.b1  a0.b2
      A2B2     integers, |a| < 2^10    integers, |b| < 2^10    a0.b0  a0.b1  a1.b0  a1.b1

      Every piece of an integer is an integer, so every piece product is one, and check_exact() asserts that sum_k of the |piece
      products| of an output element stays below 2^24: every partial sum, in any order and of any subset, is then an integer below
      2^24 and exact in float32.  The dropped products a1.b2, a2.b1, a2.b2 are zero because the pieces they need are zero (asserted).
      A missing, doubled or swapped piece product changes the sum, because the piece it belongs to is non-zero in at least a fifth
      of the entries (asserted).  For K > 16 the operand with the small values (A3B1: B, A1B3: A, A2B2: A) has at most 16 non-zeros
      per row, at positions drawn over the whole of K, so the bound holds at any K while every K tile carries terms.

  general / check_scale   uniform operands on a 2^-24 grid and the host-side conditions under which a power-of-two scale of the
                      operands commutes with every operation of the product.

B is always [N, K] here (the transB = 1 operand); the k-major operand is its transpose."""
import zlib

import numpy as np

FAMILIES = ("A3B1", "A1B3", "A2B2")
WIDE_BITS, MID_BITS, DENSE_K = 19, 10, 16
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the split
def bf16_rne(x):
    """float32 -> nearest bf16 (ties to even, on the bit pattern; overflow to Inf) -> float32.  NaN stays NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    r = np.where(np.isnan(x), np.uint64(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape)


def split3(x):
    """(x0, x1, x2) as float32 arrays holding bf16 values."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = bf16_rne(x)
        r1 = (x - x0).astype(np.float32)
        x1 = bf16_rne(r1)
        r2 = (r1 - x1).astype(np.float32)
        x2 = bf16_rne(r2)
    return x0, x1, x2


def kept_terms64(A, B):
    """sum over i + j <= 2 of A_i . B_j^T in float64 (A [M, K], B [N, K])."""
    a, b = [p.astype(np.float64) for p in split3(A)], [p.astype(np.float64) for p in split3(B)]
    out = np.zeros((A.shape[0], B.shape[0]), dtype=np.float64)
    for i in range(3):
        for j in range(3 - i):
            out += a[i] @ b[j].T
    return out


def absum(A, B):
    return np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(np.asarray(B, dtype=np.float64)).T


def product64(A, B):
    return np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64).T


def error_bound(A, B):
    """K * 2^-24 * absum: the worst case of a float32 chain of K roundings, per element."""
    return A.shape[1] * U24 * absum(A, B)


# ------------------------------------------------------------------------------------------------ exact families
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ints(rng, shape, bits):
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=shape).astype(np.float32)


def _wide_ints(rng, shape):
    """2^18 <= |a| < 2^19, either sign: all three pieces are in use (the third is non-zero in about half of such values)."""
    mag = rng.integers(1 << (WIDE_BITS - 1), 1 << WIDE_BITS, size=shape)
    return (mag * rng.choice([-1, 1], size=shape)).astype(np.float32)


def _sparse_rows(rng, X):
    """Keep at most DENSE_K entries per row of X, at positions drawn without replacement over the whole row."""
    rows, K = X.shape
    if K <= DENSE_K:
        return X
    keep = np.argsort(rng.random((rows, K)), axis=1)[:, :DENSE_K]
    mask = np.zeros((rows, K), dtype=bool)
    np.put_along_axis(mask, keep, True, axis=1)
    return np.where(mask, X, np.float32(0))


def exact_family(family, M, N, K, seed=0):
    """(A [M, K], B [N, K], C [M, N]): float32 operands of the family and the int64 product A . B^T as float32.  The conditions
    the equality rests on are asserted (check_exact)."""
    rng = _rng(family, M, N, K, seed)
    if family == "A3B1":
        A, B = _wide_ints(rng, (M, K)), _sparse_rows(rng, _ints(rng, (N, K), 1))
    elif family == "A1B3":
        A, B = _sparse_rows(rng, _ints(rng, (M, K), 1)), _wide_ints(rng, (N, K))
    elif family == "A2B2":
        A, B = _sparse_rows(rng, _ints(rng, (M, K), MID_BITS)), _ints(rng, (N, K), MID_BITS)
    else:
        raise ValueError(family)
    check_exact(family, A, B)
    C = A.astype(np.int64) @ B.astype(np.int64).T
    return A, B, C.astype(np.float32)


def share_nonzero(x):
    return float(np.count_nonzero(x)) / max(1, x.size)


def check_exact(family, A, B):
    """Assert the conditions under which the device result must equal the integer product (module docstring).  Returns the figures."""
    assert np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B)), "operands must be integers"
    a, b = split3(A), split3(B)
    for p in a + b:
        assert np.array_equal(p, np.rint(p))
    assert np.array_equal(sum(p.astype(np.float64) for p in a), A) and np.array_equal(sum(p.astype(np.float64) for p in b), B)
    top = float(absum(A, B).max()) if A.size and B.size else 0.0
    assert top < 2.0 ** 24, f"{family}: max absum {top:.3e} >= 2^24"
    # the same over the pieces: what an accumulator can hold after any subset of the kept piece products
    pieces = sum(absum(a[i], b[j]) for i in range(3) for j in range(3 - i))
    assert float(pieces.max()) < 2.0 ** 24, f"{family}: max sum of |piece products| {float(pieces.max()):.3e} >= 2^24"
    if family == "A3B1":
        wide, narrow, used = a, b, (A, B)
    elif family == "A1B3":
        wide, narrow, used = b, a, (B, A)
    else:
        wide = narrow = None
    if wide is not None:
        assert np.abs(used[0]).max() < 2 ** WIDE_BITS and np.abs(used[1]).max() <= 1
        share = share_nonzero(wide[2])
        assert share >= 0.2 and share_nonzero(wide[1]) >= 0.2, f"{family}: the third piece is non-zero in only {share:.0%} of the wide operand"
        assert not narrow[1].any() and not narrow[2].any(), f"{family}: the narrow operand has a second or third piece"
        nnz = np.count_nonzero(used[1], axis=1)
    else:
        assert np.abs(A).max() < 2 ** MID_BITS and np.abs(B).max() < 2 ** MID_BITS
        # A is the sparse one: its share counts among the entries it keeps
        share = min(float(np.count_nonzero(a[1])) / max(1, np.count_nonzero(A)), share_nonzero(b[1]))
        assert share >= 0.2, f"{family}: a second piece is non-zero in only {share:.0%} of an operand"
        assert not a[2].any() and not b[2].any(), f"{family}: an operand has a third piece"
        nnz = np.count_nonzero(A, axis=1)
    assert nnz.max() <= DENSE_K or A.shape[1] <= DENSE_K
    # every K tile of 16 carries a term somewhere: a kernel that skipped one would change the result
    for t in range(0, A.shape[1], DENSE_K):
        assert (A[:, t:t + DENSE_K] != 0).any() and (B[:, t:t + DENSE_K] != 0).any(), f"{family}: K tile at {t} is empty"
    return {"max_absum": top, "share": share}


# ------------------------------------------------------------------------------------------------ general data and the scale
def general(seed, shape, scale=1.0):
    """Uniform float32 values on the 2^-24 grid in (-1, 1), times `scale` (a power of two, so the product is exact)."""
    assert np.frexp(scale)[0] == 0.5, "scale must be a power of two"
    v = _rng("general", seed, tuple(shape)).integers(-(1 << 24) + 1, 1 << 24, size=shape)
    return (v.astype(np.float32) * np.float32(U24) * np.float32(scale)).astype(np.float32)


def quantum(X):
    """The largest power of two of which every entry of X is a multiple."""
    X = np.asarray(X, dtype=np.float64)
    nz = X[X != 0]
    assert nz.size and np.isfinite(nz).all()
    m, e = np.frexp(nz)                                 # |m| in [0.5, 1): m * 2^53 is an integer
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)   # trailing zeros
    return 2.0 ** int((e.astype(np.int64) - 53 + low).min())


def smallest_nonzero_piece(X):
    return min(float(np.abs(p[p != 0]).min()) for p in split3(X) if p.any())


def check_scale(A, B, p, q):
    """Assert that gemm_split(A * 2^p, B * 2^q) == ldexp(gemm_split(A, B), p + q) must hold bit for bit: rounding to bf16, the two
    subtractions, every piece product and every float32 accumulation commute with a power-of-two scale as long as no operand,
    piece, product or partial sum leaves the normal range, in the scaled run or the plain one."""
    for s, t in ((0, 0), (p, q)):
        f = 2.0 ** (s + t)
        # every piece is a multiple of its operand's quantum, so every piece product and every non-zero partial sum of piece
        # products, rounded or not, is a multiple of (and at least) the product of the two quanta
        assert quantum(A) * quantum(B) * f >= 2.0 ** -126
        assert smallest_nonzero_piece(A) * smallest_nonzero_piece(B) * f >= 2.0 ** -126
        assert smallest_nonzero_piece(A) * 2.0 ** s >= 2.0 ** -126 and smallest_nonzero_piece(B) * 2.0 ** t >= 2.0 ** -126
        assert float(absum(A, B).max()) * f < 2.0 ** 127
        assert float(np.abs(A).max()) * 2.0 ** s < 2.0 ** 126 and float(np.abs(B).max()) * 2.0 ** t < 2.0 ** 126


def scaled(X, p):
    out = np.ldexp(np.asarray(X, dtype=np.float32), p).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.asarray(X, dtype=np.float64) * 2.0 ** p)
    return out


# ------------------------------------------------------------------------------------------------ the shapes of the GPU file
MS, NS, KS = (1, 127, 128, 129, 300), (128, 256, 384, 512), (16, 32, 48)
EXACT_SHAPES = ([(M, N, 16) for N in (128, 256) for M in MS]            # every M on the 128-wide and the 256-wide tile, prologue only
                + [(129, N, 48) for N in NS]                            # every N, an odd tile count
                + [(129, 256, 32), (300, 384, 32)]                      # an even tile count
                + [(300, 256, 1024), (129, 512, 1024)])                 # the long cases
GENERAL_SHAPES = ((129, 128, 16), (300, 256, 64), (257, 384, 256), (130, 512, 1024))
SCALE_SHAPE, SCALES = (129, 256, 64), ((40, 40), (-20, -20), (60, -60))
NONFINITE_SHAPE = (129, 256, 32)


def general_pair(M, N, K, seed=0):
    """(X [M, K], W [N, K] scaled by K^-1/2) of the general tests; K is a power of four there, so the scale is a power of two."""
    return general((seed, "x"), (M, K)), general((seed, "w"), (N, K), scale=K ** -0.5)
