"""CPU tests of tests/gemm_split_ref.py, the reference of the split-precision product's GPU tests (no GPU needed): the bf16 rounding
against torch's cast, the properties of the three-way split, the size of the dropped terms, and the asserted conditions of every
exact family at every shape tests/test_gpu_gemm_split.py uses."""
import numpy as np
import pytest
import torch

from tests import gemm_split_ref as S


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def torch_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def wide_range(n, seed, lo=-126, hi=127):
    """n float32 values with random signs, uniform exponents in [lo, hi] and random 24-bit significands."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1 << 23, 1 << 24, size=n).astype(np.float64) * 2.0 ** -23
    x = np.ldexp(m, rng.integers(lo, hi + 1, size=n)) * rng.choice([-1.0, 1.0], size=n)
    out = x.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)
    return out


def test_bf16_rne_equals_torch_cast():
    x = wide_range(100_000, 1)
    assert np.array_equal(bits(S.bf16_rne(x)), bits(torch_bf16(x)))
    hi = np.arange(0x3F80, 0x3FA0, dtype=np.uint32) << 16          # bf16 values with an even and an odd last bit
    special = np.concatenate([
        from_bits(hi | 0x8000), from_bits(hi | 0x8000 | 0x80000000),                         # exact ties: to even and away from odd
        from_bits(hi | 0x7FFF), from_bits(hi | 0x8001),                                      # one bit either side of a tie
        from_bits([0x00000000, 0x80000000]),                                                 # +-0
        from_bits([0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807F8000, 0x00400000, 0x80000001]),  # subnormals
        from_bits([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000]),             # the largest finite float32 and bf16
        from_bits([0x7F800000, 0xFF800000]),                                                 # +-Inf
    ])
    got, ref = S.bf16_rne(special), torch_bf16(special)
    assert np.array_equal(bits(got), bits(ref)), [(hex(a), hex(b), hex(c)) for a, b, c in zip(bits(special), bits(got), bits(ref)) if b != c]
    # ties land on the even neighbour; the largest finite float32 rounds to Inf
    t = S.bf16_rne(from_bits(hi | 0x8000))
    assert not ((bits(t) >> 16) & 1).any() and np.array_equal(bits(t) >> 16, (hi >> 16) + ((hi >> 16) & 1))
    assert np.isposinf(S.bf16_rne(from_bits([0x7F7FFFFF]))[0]) and np.isneginf(S.bf16_rne(from_bits([0xFF7FFFFF]))[0])
    assert np.array_equal(bits(S.bf16_rne(from_bits([0x7F800000, 0xFF800000]))), np.array([0x7F800000, 0xFF800000], dtype=np.uint32))
    nan = from_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001])
    assert np.isnan(S.bf16_rne(nan)).all() and np.isnan(torch_bf16(nan)).all()


def test_split3_is_exact_and_each_piece_is_a_bf16_number():
    # |x| >= 2^-100: the third piece, 2^-24 |x| at the smallest, is normal or zero
    x = np.concatenate([wide_range(100_000, 2, lo=-100, hi=126), S.general(3, (50_000,)), np.float32([1.0, -1.0, 0.0, 255.0, 257.0, 2.0 ** 19 - 1])])
    p = S.split3(x)
    third_ok = (p[2] == 0) | (np.abs(p[2]) >= 2.0 ** -126)
    assert third_ok.all()
    assert np.array_equal(sum(v.astype(np.float64) for v in p), x.astype(np.float64))
    for v in p:
        assert not (bits(v) & 0xFFFF).any()                       # sign, 8 exponent bits, 7 stored significand bits + the hidden one
    assert np.all(np.abs(p[1]) <= np.abs(x) * 2.0 ** -8) and np.all(np.abs(p[2]) <= np.abs(x) * 2.0 ** -16)
    assert S.share_nonzero(p[2][:100_000]) > 0.9
    # an Inf gives NaN pieces (inf - inf), a NaN stays one
    for bad in (np.inf, -np.inf, np.nan):
        q = S.split3(np.float32([bad]))
        assert not np.isfinite(q[0][0]) and np.isnan(q[1][0]) and np.isnan(q[2][0])


@pytest.mark.parametrize("M,N,K", [(64, 48, 16), (33, 40, 256)])
def test_kept_terms_are_within_three_roundings_of_the_product(M, N, K):
    for A, B in (S.general_pair(M, N, K), (wide_range(M * K, 5, -20, 20).reshape(M, K), wide_range(N * K, 6, -20, 20).reshape(N, K))):
        err = np.abs(S.kept_terms64(A, B) - S.product64(A, B))
        bound = 3 * S.U24 * S.absum(A, B)
        assert (err <= bound).all(), float((err / bound).max())
        assert err.max() > 0                                           # the dropped terms exist: the six kept ones are not everything
    # on bf16 operands the single product a0.b0 is everything
    A, B = S.bf16_rne(A), S.bf16_rne(B)
    assert np.array_equal(S.kept_terms64(A, B), S.product64(A, B))


@pytest.mark.parametrize("family", S.FAMILIES)
def test_exact_families_meet_their_conditions_at_every_gpu_shape(family):
    for M, N, K in S.EXACT_SHAPES:
        A, B, C = S.exact_family(family, M, N, K)                       # asserts check_exact
        assert A.shape == (M, K) and B.shape == (N, K) and C.shape == (M, N) and A.dtype == B.dtype == C.dtype == np.float32
        fig = S.check_exact(family, A, B)
        assert fig["max_absum"] < 2.0 ** 24 and fig["share"] >= 0.2
        assert np.array_equal(C.astype(np.float64), S.product64(A, B)) and np.array_equal(C.astype(np.float64), S.kept_terms64(A, B))
        assert C.any()
        if K > S.DENSE_K:
            sparse = B if family == "A3B1" else A
            assert np.count_nonzero(sparse, axis=1).max() <= S.DENSE_K
    # the shapes the issue's figures were taken at
    for M, N, K in ((130, 128, 16), (130, 128, 1024), (130, 256, 256)):
        S.exact_family(family, M, N, K)


def test_exact_family_pins_every_kept_piece_product():
    """Each of the kept piece products changes the result of some family when it is left out or issued twice, and each dropped one
    is zero there: the equality test of the GPU file sees a wrong term."""
    seen = set()
    for family in S.FAMILIES:
        A, B, C = S.exact_family(family, 129, 128, 48)
        a, b = [p.astype(np.float64) for p in S.split3(A)], [p.astype(np.float64) for p in S.split3(B)]
        for i in range(3):
            for j in range(3):
                term = a[i] @ b[j].T
                if i + j > 2:
                    assert not term.any()
                elif term.any():
                    seen.add((i, j))
                    assert (C - term != C).any()
    assert seen == {(i, j) for i in range(3) for j in range(3 - i)}


def test_scale_conditions_hold_for_the_gpu_cases_and_catch_a_range_exit():
    M, N, K = S.SCALE_SHAPE
    A, B = S.general_pair(M, N, K)
    assert S.quantum(A) >= 2.0 ** -24 and S.quantum(B) >= 2.0 ** -27
    assert S.quantum(np.float32([0.75, 2.0, -0.375])) == 0.125
    for p, q in S.SCALES:
        S.check_scale(A, B, p, q)
        assert np.array_equal(S.scaled(A, p).astype(np.float64), A.astype(np.float64) * 2.0 ** p)
    with pytest.raises(AssertionError):
        S.check_scale(A, B, -50, -50)                                   # piece products below 2^-126
    with pytest.raises(AssertionError):
        S.check_scale(A, B, 70, 60)                                     # sums above 2^127


def test_general_data_is_on_the_grid():
    for M, N, K in S.GENERAL_SHAPES:
        A, B = S.general_pair(M, N, K)
        for X, g in ((A, 2.0 ** 24), (B, 2.0 ** 24 * K ** 0.5)):
            v = X.astype(np.float64) * g
            assert np.array_equal(v, np.rint(v)) and np.abs(v).max() < 2 ** 24 and X.dtype == np.float32
        assert S.error_bound(A, B).shape == (M, N)
