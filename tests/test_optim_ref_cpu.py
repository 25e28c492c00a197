"""CPU tests of tests/optim_ref.py, the restatement tests/test_gpu_optim.py holds the optimiser kernels to: every update pinned to
hand-written float32 bit patterns (worked out operation by operation, away from NumPy's array arithmetic) and to scalar loops; proofs
that the GPU comparisons can fail -- three wrongly associated variants differ in bits; and the exactness condition of the norm inputs
on every table the GPU file uses."""
import math

import numpy as np

from tests import norm_ref as R
from tests import optim_ref as O

F32 = np.float32

P = np.array([0.5, -1.25, 0.3, 2.0], dtype=np.float32)
G = np.array([0.1, -0.2, 0.7, -0.05], dtype=np.float32)
G_NEXT = np.array([-0.3, 0.4, 0.05, 0.6], dtype=np.float32)
Z = np.zeros(4, dtype=np.float32)
LR, B1, B2, EPS, WD = 0.01, 0.9, 0.999, 1e-8, 0.05


def lit(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def test_one_adam_step_from_zero_state():
    """Coupled decay: g2 = g + 0.05 p; c1 = 1 - 0.9f = 0x3DCCCCD0, c2 = 1 - 0.999f."""
    p, m, v = O.adam_ref(P, G, Z, Z, LR, B1, B2, EPS, 1, wd=WD)
    R.assert_bits(p, lit(0x3EFAE148, 0xBF9EB852, 0x3E947AE2, 0x3FFEB852), "p")
    R.assert_bits(m, lit(0x3C4CCCD0, 0xBCD70A40, 0x3D926E99, 0x3BA3D70D), "m")
    R.assert_bits(v, lit(0x37831200, 0x38908148, 0x3A060349, 0x3627C51F), "v")
    c1, c2 = O.bias_corrections(B1, B2, 1)
    assert R.same_bits(c1, lit(0x3DCCCCD0)[0]) and float(c2) == float(F32(1.0 - float(F32(0.999))))


def test_one_adamw_step_from_zero_state():
    """Decoupled: the moments see the raw gradient (m = (1 - 0.9f) g), the parameter shrinks by (lr * wd) * p before the update."""
    p, m, v = O.adam_ref(P, G, Z, Z, LR, B1, B2, EPS, 1, wd=WD, decoupled=True)
    R.assert_bits(p, lit(0x3EFAC083, 0xBF9EA3D7, 0x3E946739, 0x40009375), "p")
    R.assert_bits(m, lit(0x3C23D70D, 0xBCA3D70D, 0x3D8F5C2B, 0xBBA3D70D), "m")
    R.assert_bits(v, lit(0x3727C51F, 0x3827C51F, 0x3A0072EB, 0x3627C51F), "v")
    # wd == 0: both forms are the same update
    a, b = O.adam_ref(P, G, Z, Z, LR, B1, B2, EPS, 1), O.adam_ref(P, G, Z, Z, LR, B1, B2, EPS, 1, decoupled=True)
    assert all(R.same_bits(x, y) for x, y in zip(a, b))


def test_two_momentum_steps_and_nesterov():
    """momentum 0.9, dampening 0.1, wd 0.05: the first buffer is g2 itself (0.1 + 0.05 * 0.5 = 0.125 exactly), the second
    0.9 buf + (1 - 0.1f) g2.  Nesterov (no dampening, no decay): d = g2 + 0.9 buf'."""
    p1, b1 = O.momentum_ref(P, G, Z, LR, 0.9, 0.1, first=True, wd=WD)
    R.assert_bits(p1, lit(0x3EFF5C29, 0xBF9FA9FC, 0x3E95F070, 0x3FFFEF9E), "p after step 1")
    R.assert_bits(b1, lit(0x3E000000, 0xBE866666, 0x3F370A3D, 0x3D4CCCCD), "buf after step 1")
    p2, b2 = O.momentum_ref(p1, G_NEXT, b1, LR, 0.9, 0.1, wd=WD)
    R.assert_bits(p2, lit(0x3F000697, 0xBF9FC024, 0x3E9258BC, 0x3FFF1271), "p after step 2")
    R.assert_bits(b2, lit(0xBE0A4C2F, 0x3D8A7B60, 0x3F33A12F, 0x3F2CCB54), "buf after step 2")
    n1, nb1 = O.momentum_ref(P, G, Z, LR, 0.9, nesterov=True, first=True)
    R.assert_bits(n1, lit(0x3EFF06F7, 0xBF9F837B, 0x3E92CA58, 0x40000F91), "nesterov p after step 1")
    R.assert_bits(nb1, G, "nesterov buf after step 1")
    n2, nb2 = O.momentum_ref(n1, G_NEXT, nb1, LR, 0.9, nesterov=True)
    R.assert_bits(n2, lit(0x3F00C3F4, 0xBFA0476F, 0x3E8F66A6, 0x3FFEB6D9), "nesterov p after step 2")
    R.assert_bits(nb2, lit(0xBE570A3E, 0x3E6147AF, 0x3F2E147B, 0x3F0E147B), "nesterov buf after step 2")


def test_updates_against_scalar_loops():
    """The array expressions against float32 scalars, one operation per line, with a scale and at a later step."""
    rng = np.random.default_rng(5)
    n = 64
    p, g = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    m, v = rng.uniform(-0.1, 0.1, n).astype(np.float32), rng.uniform(0.01, 0.1, n).astype(np.float32)
    lr, b1, b2, eps, wd, s = F32(LR), F32(B1), F32(B2), F32(EPS), F32(WD), F32(0.37)
    c1, c2 = O.bias_corrections(B1, B2, 7)
    for decoupled in (False, True):
        gp, gm, gv = O.adam_ref(p, g, m, v, LR, B1, B2, EPS, 7, wd=WD, decoupled=decoupled, scale=s)
        for i in range(n):
            g2 = g[i] * s
            if not decoupled:
                g2 = g2 + wd * p[i]
            m1 = b1 * m[i] + (F32(1) - b1) * g2
            v1 = b2 * v[i] + ((F32(1) - b2) * g2) * g2
            u = (m1 / c1) / (F32(math.sqrt(float(v1 / c2))) + eps)        # sqrt in float64, rounded: correctly rounded float32 sqrt
            pi = p[i] - (lr * wd) * p[i] if decoupled else p[i]
            assert R.same_bits(gp[i], pi - lr * u) and R.same_bits(gm[i], m1) and R.same_bits(gv[i], v1)
    mo, da = F32(0.9), F32(0.25)
    for nesterov in (False, True):
        gp, gb = O.momentum_ref(p, g, m, LR, 0.9, 0.25, nesterov=nesterov, wd=WD, scale=s)
        for i in range(n):
            g2 = g[i] * s + wd * p[i]
            bb = mo * m[i] + (F32(1) - da) * g2
            d = g2 + mo * bb if nesterov else bb
            assert R.same_bits(gp[i], p[i] - lr * d) and R.same_bits(gb[i], bb)


def test_wrongly_associated_variants_differ_in_bits():
    """(1 - b2) * (g * g), a fused b1 * m + ..., and lr * wd applied after the update are equal to the contract in exact arithmetic and
    differ from it somewhere on 10^5 elements: the GPU comparison tells them apart."""
    rng = np.random.default_rng(6)
    n = 100_000
    p, g = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    m, v = rng.uniform(-0.1, 0.1, n).astype(np.float32), rng.uniform(0.01, 0.1, n).astype(np.float32)
    ref = O.adam_ref(p, g, m, v, LR, B1, B2, EPS, 3)
    sq = O.adam_square_first(p, g, m, v, LR, B1, B2, EPS, 3)
    assert (R.bits(ref[2]) != R.bits(sq[2])).any() and np.array_equal(R.bits(ref[1]), R.bits(sq[1]))
    fused = O.adam_fused_m(p, g, m, v, LR, B1, B2, EPS, 3)
    assert (R.bits(ref[1]) != R.bits(fused[1])).any() and np.array_equal(R.bits(ref[2]), R.bits(fused[2]))
    refw = O.adam_ref(p, g, m, v, LR, B1, B2, EPS, 3, wd=WD, decoupled=True)
    last = O.adamw_decay_last(p, g, m, v, LR, B1, B2, EPS, 3, WD)
    assert (R.bits(refw[0]) != R.bits(last[0])).any() and np.array_equal(R.bits(refw[1]), R.bits(last[1]))
    assert np.abs(refw[0] - last[0]).max() < 1e-6     # ... by roundings only


def test_momentum_zero_is_sgd():
    """momentum = 0, dampening = 0: p - lr * (g + wd * p), the bits of elementwise_ref.sgd_ref -- g = -0 and an infinite p included,
    on the first step (buf' = g2) and on a later one over a +0 buffer."""
    from tests.elementwise_ref import sgd_ref
    rng = np.random.default_rng(7)
    p, g = rng.uniform(-1, 1, 300).astype(np.float32), rng.uniform(-1, 1, 300).astype(np.float32)
    p[:3], g[:3] = (np.inf, -np.inf, 0.0), (1.0, -0.0, -0.0)
    for wd in (0.0, 5e-4):
        for first in (True, False):
            got, buf = O.momentum_ref(p, g, np.zeros_like(p), 0.1, 0.0, first=first, wd=wd)
            R.assert_bits(got, sgd_ref(p, g, 0.1, wd), f"wd={wd} first={first}")


def test_zero_gradient_on_zero_state_and_subnormal_guard():
    p = np.array([0.0, -0.0, 1.5, -2.0], dtype=np.float32)
    for wd, dec in ((0.0, False), (0.05, True)):
        got, m, v = O.adam_ref(p, Z, Z, Z, LR, B1, B2, EPS, 1, wd=wd, decoupled=dec)
        assert R.same_bits(m, Z) and R.same_bits(v, Z)
        if wd == 0.0:
            R.assert_bits(got, p, "p")          # 0 / (sqrt(0) + eps) = 0: p - lr * 0
    O.no_subnormals(*O.adam_intermediates(P, G, Z, Z, LR, B1, B2, EPS, 1, wd=WD))
    try:
        O.no_subnormals(np.array([1e-40], dtype=np.float32))
    except AssertionError:
        pass
    else:
        raise AssertionError("no_subnormals let a subnormal through")


def test_bias_corrections():
    for b in (0.9, 0.999, 0.0):
        for t in (1, 2, 10, 1000):
            c = O.bias_corrections(b, b, t)[0]
            assert c.dtype == np.float32 and float(c) == float(F32(1.0 - float(F32(b)) ** t))
    assert float(O.bias_corrections(0.0, 0.0, 1)[0]) == 1.0 and 0.0 < float(O.bias_corrections(0.999, 0.999, 1)[0]) < 0.0011


def test_norm_inputs_are_exact_on_every_table():
    """Gradients from {+-2^-1 .. +-2^-4}: every square a multiple of 2^-8, the sum below 2^24 quanta (asserted by sqnorm_exact_ref), and
    equal to the float64 sum in any order; a dropped or doubled element changes it."""
    for sizes in (O.TABLE_ONE, O.TABLE_NINE, O.TABLE_MANY):
        grads = O.norm_gradients(sizes)
        assert [len(g) for g in grads] == list(sizes) and all(g.dtype == np.float32 for g in grads)
        ref = O.sqnorm_exact_ref(grads)
        flat = np.concatenate(grads)
        assert float(ref) == float((flat.astype(np.float64) ** 2).sum())
        acc = F32(0)
        for x in flat[np.random.default_rng(1).permutation(len(flat))]:
            acc = acc + x * x
        assert acc == ref
        assert float(O.sqnorm_exact_ref([flat[1:]])) != float(ref)
    # the scale: above the norm 1, below it max_norm / (norm + 1e-6) with three roundings
    sq = O.sqnorm_exact_ref(O.norm_gradients(O.TABLE_NINE))
    norm = F32(math.sqrt(float(sq)))
    assert O.gscale_ref(sq, float(norm) * 2) == F32(1)
    assert R.same_bits(O.gscale_ref(sq, 0.5), F32(0.5) / (norm + F32(1e-6))) and O.gscale_ref(sq, 0.5) < 1
    assert O.state_offsets((1, 3, 4, 5, 0, 1023)) == ([0, 4, 8, 12, 20, 20], 1044)
