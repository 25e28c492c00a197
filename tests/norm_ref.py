"""NumPy restatement of the BatchNorm + ReLU kernels (gnn.cpp_amd/csrc/gnnx_norm.hip) and the two kinds of reference the
BatchNorm and elementwise tests hold the kernels to (tests/test_gpu_norm.py, tests/test_gpu_elementwise.py).

(a) ELEMENT ARITHMETIC is restated in float32 with one rounding per operation, in the kernels' association.  The kernel files
    switch floating-point contraction off and the build has no fast-math, IEEE add / sub / mul / div / sqrt are correctly rounded
    on both sides, so a NumPy float32 expression of the same shape gives the same bits.  Compared with `same_bits` (NaN equals
    NaN); a swapped association fails.

(b) REDUCTIONS are checked on inputs whose sum is exact in float32 in ANY order, so that the order (grid, slots, unrolling) stays
    a performance detail.  The condition, per output column:

        sum_i |term_i| / quantum < 2^24,      quantum = a power of two that divides every term

    Every partial sum of any subset in any order is then a multiple of `quantum` below 2^24 quanta, which float32 holds exactly;
    the reference is the float64 sum cast to float32 and the comparison is equality.  `exact_colsum` asserts the condition for
    every matrix of terms it sums: a generator that breaks it is a test bug, never a tolerance.

    What a lost row changes.  x and dy have no zeros, so a dropped or doubled row changes EVERY column of the sums of x and of g
    (before the ReLU mask).  The two centred sums, (x - mean)^2 and g * xhat, have that property in the columns with mean = +-0.5
    only: the columns with mean = +-1 (half of them, there for the +-0 forward values of the ReLU edge) hold a zero term wherever
    x == mean, a quarter of their rows, and a row lost there shows in the other columns.  Every width above 2 has both kinds.

    Rounding leg (real-valued data, n <= 300 only): any-order bound gamma_k * sum|term| with gamma_k = k u / (1 - k u), u = 2^-24,
    k = the number of roundings on the longest path to the result (`gamma_k`)."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
X_VALUES = np.array([-2, -1, 1, 2], dtype=np.float32)                      # no zeros: a dropped row changes every column sum of x, g
MEAN_VALUES = np.array([-0.5, 0.5, 1.0, -1.0], dtype=np.float32)           # +-1: x == mean happens (forward value +-0, a zero centred term)
VAR_VALUES = np.array([0.25, 1.0, 4.0], dtype=np.float32)                  # eps = 0: sigma and 1 / sigma in {0.5, 1, 2}, exact
GAMMA_VALUES = np.array([1.0, -2.0, 0.5, -1.0, 2.0], dtype=np.float32)
BETA_VALUES = np.array([0.0, -0.0, -0.5, 0.25, 1.0, -2.0, 0.0], dtype=np.float32)
QUANTUM = 0.25                                                              # divides x, (x - mean)^2, g, g * xhat of exact_case


def f32(a):
    return np.asarray(a, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """Equal bit patterns, a NaN equal to any NaN (payloads are not compared)."""
    a, b = f32(a), f32(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def describe_mismatch(got, ref):
    got, ref = f32(got), f32(ref)
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    bad = ~((bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref)))
    if not bad.any():
        return None
    idx = tuple(int(v) for v in np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} elements differ, first at {idx}: got {got[idx]!r}, expected {ref[idx]!r}"


def assert_bits(got, ref, what):
    msg = describe_mismatch(got, ref)
    assert msg is None, f"{what}: {msg}"


def gamma_k(k):
    """The standard bound (1 + u)^k - 1 <= k u / (1 - k u) of k float32 roundings."""
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------- (b) exact reductions
def check_exact(terms, quantum=QUANTUM):
    """Assert the exactness condition of the module docstring for the columns of `terms` ([n, F], any float type)."""
    t = np.asarray(terms, dtype=np.float64).reshape(-1, np.shape(terms)[-1])
    q = t / quantum
    assert np.array_equal(q, np.rint(q)), f"a term is not a multiple of the quantum {quantum}"
    worst = np.abs(q).sum(0).max() if t.size else 0.0
    assert worst < 2.0 ** 24, f"sum|term| / quantum = {worst:.0f} >= 2^24: the column sum is not exact in every order"


def exact_colsum(terms, quantum=QUANTUM, scale=1.0):
    """float32(scale * sum_i terms[i, :]) of terms that meet the condition (asserted); scale is a power of two."""
    check_exact(terms, quantum)
    assert np.frexp(scale)[0] == 0.5, "scale must be a power of two"
    s = np.asarray(terms).reshape(-1, np.shape(terms)[-1]).sum(0, dtype=np.float64) * scale
    out = s.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), s)
    return out


def exact_case(n, F, seed=0):
    """Inputs of the exact legs: x, dy in {-2, -1, 1, 2}; per-column mean, var, gamma, beta from the value tables above (periods 4,
    3, 5 and 7 in the column index, shifted by the seed, so every combination turns up within 420 columns), eps = 0.  Every forward
    value (x - mean) / sigma * gamma + beta is dyadic and exact; columns with mean = +-1 meet x == mean, where the forward value is
    +0 or -0 (negative gamma, beta -0 or absent) -- the `v > 0` edge of the ReLU -- and negative betas push whole columns below it."""
    rng = np.random.default_rng([seed, n, F])
    col = np.arange(F) + seed
    return dict(x=X_VALUES[rng.integers(0, 4, (n, F), dtype=np.uint8)], dy=X_VALUES[rng.integers(0, 4, (n, F), dtype=np.uint8)], mean=MEAN_VALUES[col % 4],
                var=VAR_VALUES[col % 3], gamma=GAMMA_VALUES[col % 5], beta=BETA_VALUES[col % 7], eps=0.0)


def random_case(n, F, seed=0):
    """Real-valued inputs of the element-arithmetic legs (statistics are whatever the caller computes or these made-up ones)."""
    rng = np.random.default_rng([seed + 77, n, F])
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return dict(x=u(n, F) * F32(2) + F32(0.3), dy=u(n, F), mean=u(F) * F32(0.5) + F32(0.3), var=u(F) * F32(0.5) + F32(1.3),
                gamma=u(F) + F32(1.5) * np.where(np.arange(F) % 3 == 0, F32(-1), F32(1)), beta=u(F) * F32(0.3), eps=1e-5)


# ---------------------------------------------------------------------------------------------- (a) element arithmetic
def bn_fwd_ref(x, mean=None, var=None, gamma=None, beta=None, eps=1e-5, relu=True):
    """y = relu(((x - mean) / sqrt(var + eps)) * gamma + beta): sub, div, mul, add, each rounded; relu = where(v > 0, v, 0).
    mean / var None: ReLU only (gamma and beta are not read then, as in the kernels)."""
    v = f32(x)
    with np.errstate(all="ignore"):
        if mean is not None:
            sd = np.sqrt(f32(var) + F32(eps))
            v = (v - f32(mean)) / sd
            if gamma is not None:
                v = v * f32(gamma)
            if beta is not None:
                v = v + f32(beta)
        if relu:
            v = np.where(v > 0, v, F32(0))
    return f32(v)


def relu_mask_ref(x, y=None, mean=None, var=None, gamma=None, beta=None, eps=1e-5):
    """Did the forward ReLU pass the element: from the stored forward output, or by redoing the forward arithmetic on x."""
    with np.errstate(invalid="ignore"):
        if y is not None:
            return f32(y) > 0
        return bn_fwd_ref(x, mean, var, gamma, beta, eps, relu=False) > 0


def masked(dy, mask):
    """g = dY where the ReLU passed, +0 elsewhere (not dY * 0: no -0, no NaN from an inf)."""
    return f32(dy) if mask is None else np.where(mask, f32(dy), F32(0))


def xhat_ref(x, mean, var, eps):
    with np.errstate(all="ignore"):
        rstd = F32(1) / np.sqrt(f32(var) + F32(eps))
        return (f32(x) - f32(mean)) * rstd, rstd


def bn_bwd_apply_ref(x, g, mean, var, gamma, dgamma, dbeta, n_total, eps=1e-5):
    """dx = (gamma * rstd) * ((g - dbeta * inv_n) - (xhat * dgamma) * inv_n), inv_n = float32(1) / float32(n_total); g is already
    masked.  mean None: the mask-only form, dx = g."""
    if mean is None:
        return f32(g)
    with np.errstate(all="ignore"):
        xhat, rstd = xhat_ref(x, mean, var, eps)
        inv_n = F32(1) / F32(n_total)
        gm = F32(1) if gamma is None else f32(gamma)
        return f32((gm * rstd) * ((f32(g) - f32(dbeta) * inv_n) - (xhat * f32(dgamma)) * inv_n))


def bn_bwd_apply_swapped(x, g, mean, var, gamma, dgamma, dbeta, n_total, eps=1e-5):
    """The same formula with the WRONG association gamma * (rstd * (...)): what the bit comparison must be able to tell apart."""
    with np.errstate(all="ignore"):
        xhat, rstd = xhat_ref(x, mean, var, eps)
        inv_n = F32(1) / F32(n_total)
        gm = F32(1) if gamma is None else f32(gamma)
        return f32(gm * (rstd * ((f32(g) - f32(dbeta) * inv_n) - (xhat * f32(dgamma)) * inv_n)))


def bn_bwd_quirk_ref(g, var, gamma, eps=1e-5):
    """dx = (g * gamma) / sqrt(var + eps): the statistics as constants."""
    with np.errstate(all="ignore"):
        v = f32(g)
        if gamma is not None:
            v = v * f32(gamma)
        return f32(v / np.sqrt(f32(var) + F32(eps)))


def bn_bwd_terms(x, g, mean, var, eps):
    """(terms of dbeta, terms of dgamma) in float64: g and g * xhat with xhat restated in float32."""
    xhat, _ = xhat_ref(x, mean, var, eps)
    g64 = np.asarray(g, dtype=np.float64)
    return g64, g64 * xhat.astype(np.float64)


def bn_stats_mean_ref(x):
    """The kernel's mean on exact data: float32(sum) * (float32(1) / float32(n))."""
    n = np.shape(x)[0]
    return exact_colsum(x) * (F32(1) / F32(n))


def sqdev_terms(x, mean):
    """(x - mean)^2 with the float32 subtraction and product of the kernel, as float64 (exact on the exact data)."""
    d = f32(x) - f32(mean)
    return (d * d).astype(np.float64)


# ---------------------------------------------------------------------------------------------- the shapes of tests/test_gpu_norm.py
# (F, pad): the matrices sit on a leading dimension F + pad.  An odd pad forces the scalar kernels at a width the 16-byte kernels
# would take; the statistics always run in colreduce_stage1 (fw = 1, 8, 64, 128, 256; two column passes at 300, five at 1028).
SCALAR_WIDTHS = ((1, 0), (7, 0), (33, 0), (100, 1), (256, 1), (300, 1), (1028, 0))
VECTOR_WIDTHS = ((4, 0), (12, 0), (100, 0), (256, 0), (300, 0), (1020, 0), (1024, 0))
BIG_CELLS = ((4, 0, 65_537, "empty-blocks-vec"), (7, 0, 65_537, "empty-blocks-scalar"), (7, 0, 100_003, "unrolled-reduce"))
APPLY_CELLS = ((1024, 0, 32_771, "8192-block-cap"), (257, 0, 4_099, "4096-block-wrap"))     # forward and apply only: no sums
MAX_ROWS = 100_003


def is_vector(F, pad):
    return F % 4 == 0 and F <= 1024 and pad % 4 == 0


def row_counts(F, pad):
    """1; 63, 64, 65 (one reduce block becomes two); for the 16-byte kernels 4 * rpp - 1, 4 * rpp, 4 * rpp + 1 with rpp = 256 / (F / 4)
    rows per pass (one pass of four rows in flight, exactly, and one more)."""
    ns = [1, 63, 64, 65]
    if is_vector(F, pad):
        rpp = 256 // (F // 4)
        ns += [4 * rpp - 1, 4 * rpp, 4 * rpp + 1]
    return sorted(set(ns))


def cells():
    """(F, pad, n, name) of every full cell (statistics, forward, both backward halves)."""
    out = [(F, pad, n, "vector" if is_vector(F, pad) else "scalar") for F, pad in SCALAR_WIDTHS + VECTOR_WIDTHS for n in row_counts(F, pad)]
    return out + list(BIG_CELLS)


def cell_id(c):
    F, pad, n, name = c
    return f"F{F}-ld{F + pad}-n{n}-{name}"
