"""NumPy restatement of the optimiser kernels of gnn.cpp_amd/csrc/gnnx_optim.hip (the contract of include/gnnx.h), in the two kinds
of reference of tests/elementwise_ref.py: element arithmetic in float32 with one rounding per operation, compared bit for bit; and the
gradient norm on inputs whose sum of squares is exact in float32 in any order, compared by equality with the float64 sum.

    g1 = g * s                       only with a scale
    g2 = g1 + wd * p                 only when wd != 0 and the decay is coupled
  Adam:      m' = b1 * m + (1 - b1) * g2;  v' = b2 * v + ((1 - b2) * g2) * g2;  u = (m' / c1) / (sqrt(v' / c2) + eps)
             p1 = p - (lr * wd) * p   only when decoupled and wd != 0;  p' = p1 - lr * u
  momentum:  buf' = g2 if first else momentum * buf + (1 - dampening) * g2;  d = g2 + momentum * buf' if nesterov else buf'
             p' = p - lr * d

NumPy's float32 division and square root are IEEE (correctly rounded), and an expression of float32 arrays and float32 scalars is
evaluated operation by operation in float32.  Subnormal intermediates are outside the contract: `no_subnormals` asserts that a case
produces none."""
import numpy as np

from tests.norm_ref import F32, f32

TINY = np.finfo(np.float32).tiny
NORM_VALUES = np.array([s * 2.0 ** -k for k in (1, 2, 3, 4) for s in (1, -1)], dtype=np.float32)    # +-2^-1 .. +-2^-4
NORM_QUANTUM = 2.0 ** -8                                                                              # divides every square

# the tables of tests/test_gpu_optim.py: tensor sizes (a chunk is 1024 elements)
TABLE_ONE = (1025,)
TABLE_NINE = (1, 3, 4, 5, 0, 1023, 1024, 1025, 2049)
TABLE_MANY = tuple(1 + k % 7 for k in range(300))


def no_subnormals(*arrays):
    """Assert that no value is a non-zero subnormal (the kernels keep denormals, but the contract leaves them out)."""
    for a in arrays:
        a = np.abs(f32(a))
        assert not ((a > 0) & (a < TINY)).any(), "a subnormal value: outside the contract"


def bias_corrections(b1, b2, t):
    """(c1, c2) = float32(1 - b^t), the power in float64 from the float32 beta: gnnx_adam_bias_corrections."""
    return tuple(F32(1.0 - float(F32(b)) ** t) for b in (b1, b2))


def _g2(p, g, wd, scale, coupled):
    if scale is not None:
        g = g * F32(scale)
    if coupled and wd != 0.0:
        g = g + F32(wd) * p
    return g


def adam_ref(p, g, m, v, lr, b1, b2, eps, t, wd=0.0, decoupled=False, scale=None):
    """(p', m', v') of step number t (1 for the first)."""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    c1, c2 = bias_corrections(b1, b2, t)
    with np.errstate(all="ignore"):
        g2 = _g2(p, g, wd, scale, not decoupled)
        m1 = b1 * m + (F32(1) - b1) * g2
        v1 = b2 * v + ((F32(1) - b2) * g2) * g2
        u = (m1 / c1) / (np.sqrt(v1 / c2) + eps)
        p1 = p - (lr * F32(wd)) * p if (decoupled and wd != 0.0) else p
        out = p1 - lr * u
    assert all(a.dtype == np.float32 for a in (g2, m1, v1, u, out))
    return out, m1, v1


def adam_intermediates(p, g, m, v, lr, b1, b2, eps, t, wd=0.0, decoupled=False, scale=None):
    """Every rounded intermediate of adam_ref, for no_subnormals."""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    c1, c2 = bias_corrections(b1, b2, t)
    with np.errstate(all="ignore"):
        g2 = _g2(p, g, wd, scale, not decoupled)
        a, b = b1 * m, (F32(1) - b1) * g2
        c, d = b2 * v, (F32(1) - b2) * g2
        m1, v1 = a + b, c + d * g2
        q, r = m1 / c1, v1 / c2
        u = q / (np.sqrt(r) + eps)
        return [g2, a, b, c, d, d * g2, m1, v1, q, r, np.sqrt(r), u, lr * u, (lr * F32(wd)) * p, F32(wd) * p]


def momentum_ref(p, g, buf, lr, momentum, dampening=0.0, nesterov=False, first=False, wd=0.0, scale=None):
    """(p', buf')."""
    p, g, buf = f32(p), f32(g), f32(buf)
    lr, mo, da = F32(lr), F32(momentum), F32(dampening)
    with np.errstate(all="ignore"):
        g2 = _g2(p, g, wd, scale, True)
        b1 = g2 if first else mo * buf + (F32(1) - da) * g2
        d = g2 + mo * b1 if nesterov else b1
        out = p - lr * d
    assert out.dtype == np.float32 and b1.dtype == np.float32
    return out, f32(b1)


# ---- wrongly associated variants: equal in exact arithmetic, told apart in bits (tests/test_optim_ref_cpu.py) ----------------------
def adam_square_first(p, g, m, v, lr, b1, b2, eps, t):
    """v' = b2 * v + (1 - b2) * (g * g)."""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    c1, c2 = bias_corrections(b1, b2, t)
    m1 = b1 * m + (F32(1) - b1) * g
    v1 = b2 * v + (F32(1) - b2) * (g * g)
    return p - lr * ((m1 / c1) / (np.sqrt(v1 / c2) + eps)), m1, v1


def adam_fused_m(p, g, m, v, lr, b1, b2, eps, t):
    """m' = fma(b1, m, (1 - b1) * g): the sum of the exact product, rounded once."""
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    c1, c2 = bias_corrections(b1, b2, t)
    m1 = (np.float64(b1) * m.astype(np.float64) + ((F32(1) - b1) * g).astype(np.float64)).astype(np.float32)   # 24 x 24 bits: exact in f64
    v1 = b2 * v + ((F32(1) - b2) * g) * g
    return p - lr * ((m1 / c1) / (np.sqrt(v1 / c2) + eps)), m1, v1


def adamw_decay_last(p, g, m, v, lr, b1, b2, eps, t, wd):
    """p' = (p - lr * u) - (lr * wd) * p: the decay applied after the update."""
    p0 = f32(p)
    out, m1, v1 = adam_ref(p0, g, m, v, lr, b1, b2, eps, t)
    return out - (F32(lr) * F32(wd)) * p0, m1, v1


# ---- the norm ---------------------------------------------------------------------------------------------------------------------------
def norm_gradients(sizes, seed=0):
    """One gradient per tensor from {+-2^-1 .. +-2^-4}: every square is a multiple of 2^-8, at most 2^-2."""
    rng = np.random.default_rng([seed, len(sizes)])
    return [NORM_VALUES[rng.integers(0, len(NORM_VALUES), n)] for n in sizes]


def sqnorm_exact_ref(grads):
    """float32 sum of squares of gradients that meet the exactness condition (asserted): sum / 2^-8 < 2^24, so every partial sum in
    any order is an integer number of quanta below 2^24 -- exact -- and the result is the float64 sum."""
    sq = np.concatenate([f32(g).astype(np.float64) ** 2 for g in grads] + [np.zeros(0)])
    q = sq / NORM_QUANTUM
    assert np.array_equal(q, np.rint(q)), "a square is not a multiple of 2^-8"
    assert q.sum() < 2.0 ** 24, "sum / 2^-8 >= 2^24: the sum is not exact in every order"
    s = sq.sum()
    out = F32(s)
    assert float(out) == s
    return out


def sqnorm_ordered_ref(grads):
    """The documented summation order on general data, in float32: chunks of 1024 elements per tensor (a tensor of size 0 has none);
    workgroup b of 256 takes chunks b, b + 256, ...; its thread i adds g^2 of elements i, i + 256, i + 512, i + 768 of each chunk in
    that order; the 256 sums fold in a tree (i += i + s for s = 128, 64, .. 1); the 256 partials are added in order."""
    acc = np.zeros((256, 256), dtype=np.float32)
    chunk = 0
    for g in grads:
        g = f32(g).ravel()
        for base in range(0, len(g), 1024):
            row = acc[chunk % 256]
            for k in range(base, min(base + 1024, len(g)), 256):
                seg = g[k:min(k + 256, base + 1024)]
                row[:len(seg)] = row[:len(seg)] + seg * seg
            chunk += 1
    s = 128
    while s:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    total = F32(0)
    for b in range(256):
        total = total + acc[b, 0]
    return total


def gscale_ref(sqnorm, max_norm):
    """min(1, max_norm / (sqrt(sq) + 1e-6)) in float32, one rounding per operation."""
    with np.errstate(all="ignore"):
        return np.minimum(F32(1), F32(max_norm) / (np.sqrt(F32(sqnorm)) + F32(1e-6)))


def state_offsets(sizes):
    """Offsets of the tensors' state in the arena (elements, each rounded up to 4) and the arena's length."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4
    return offs, off
