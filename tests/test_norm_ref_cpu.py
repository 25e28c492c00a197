"""CPU tests of tests/norm_ref.py, the restatement tests/test_gpu_norm.py holds the BatchNorm kernels to: the element arithmetic
against float64 autograd of relu(bn(x)) and against plain Python loops; the exact inputs meet the exactness condition at every
shape the GPU file uses; and the GPU comparisons can fail (a shuffled order changes nothing, a dropped or doubled row changes every
column, a swapped association changes bits)."""
import numpy as np
import pytest

from tests import norm_ref as R
from tests.helpers import assert_close

F32 = np.float32


def stats64(x):
    x64 = x.astype(np.float64)
    return x64.mean(0).astype(np.float32), x64.var(0).astype(np.float32)


@pytest.mark.parametrize("n,F,relu,use_gamma,use_beta", [(40, 5, True, True, True), (64, 12, True, True, False), (33, 7, False, True, True),
                                                          (50, 4, True, False, False)])
def test_restatement_matches_float64_autograd(n, F, relu, use_gamma, use_beta):
    """Forward and textbook backward of the restatement against torch float64 autograd of relu(bn(x)) with batch statistics, at the
    bars of tests/test_gpu_parity.py (forward 1e-5 * max(1, |ref|); sums 1e-5 * max(1, sum|term|); dX 1e-4 * max(1, max|dX|))."""
    import torch
    c = R.random_case(n, F, seed=1)
    x, dy, eps = c["x"], c["dy"], 1e-5
    gamma = c["gamma"] if use_gamma else None
    beta = c["beta"] if use_beta else None
    mean, var = stats64(x)
    y = R.bn_fwd_ref(x, mean, var, gamma, beta, eps, relu)
    mask = R.relu_mask_ref(x, y) if relu else None
    assert np.array_equal(mask, R.relu_mask_ref(x, None, mean, var, gamma, beta, eps)) if relu else True
    g = R.masked(dy, mask)
    t0, t1 = R.bn_bwd_terms(x, g, mean, var, eps)
    dbeta, dgamma = t0.sum(0).astype(np.float32), t1.sum(0).astype(np.float32)
    dx = R.bn_bwd_apply_ref(x, g, mean, var, gamma, dgamma, dbeta, n, eps)

    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma if use_gamma else np.ones(F), dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta if use_beta else np.zeros(F), dtype=torch.float64, requires_grad=True)
    v = (xt - xt.mean(0)) / torch.sqrt(xt.var(0, unbiased=False) + eps) * gt + bt
    yt = torch.relu(v) if relu else v
    yt.backward(torch.tensor(dy, dtype=torch.float64))
    assert_close(y, yt.detach().numpy().astype(np.float32), "forward")
    if relu:    # the comparison is only meaningful where float32 and float64 agree on the sign
        assert np.array_equal(mask, (v > 0).numpy()), "a forward value within rounding of 0: pick another seed"
    assert np.abs(dbeta - bt.grad.numpy()).max() <= 1e-5 * max(1.0, np.abs(t0).sum(0).max())
    assert np.abs(dgamma - gt.grad.numpy()).max() <= 1e-5 * max(1.0, np.abs(t1).sum(0).max())
    ref = xt.grad.numpy()
    assert np.abs(dx - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_restatement_matches_plain_loops():
    """Every vectorised expression of the restatement against a loop over the elements in float32 scalars, bit for bit: the exact
    data (with its +-0 forward values) and random data, every pointer mode."""
    for case, n, F in ((R.exact_case(9, 40, seed=2), 9, 40), (R.random_case(6, 5, seed=3), 6, 5)):
        x, dy, mean, var, eps = case["x"], case["dy"], case["mean"], case["var"], case["eps"]
        dgamma, dbeta = (np.arange(F) % 5 - 2).astype(np.float32), (np.arange(F) % 3 - 1).astype(np.float32) * F32(0.5)
        for gamma in (case["gamma"], None):
            for beta in (case["beta"], None):
                y0 = R.bn_fwd_ref(x, mean, var, gamma, beta, eps, relu=False)
                y1 = R.bn_fwd_ref(x, mean, var, gamma, beta, eps, relu=True)
                g = R.masked(dy, R.relu_mask_ref(x, None, mean, var, gamma, beta, eps))
                dx = R.bn_bwd_apply_ref(x, g, mean, var, gamma, dgamma, dbeta, 16, eps)
                dq = R.bn_bwd_quirk_ref(g, var, gamma, eps)
                for i in range(n):
                    for f in range(F):
                        sd = np.sqrt(var[f] + F32(eps))
                        v = (x[i, f] - mean[f]) / sd
                        if gamma is not None:
                            v = v * gamma[f]
                        if beta is not None:
                            v = v + beta[f]
                        assert R.same_bits(y0[i, f], v)
                        assert R.same_bits(y1[i, f], v if v > 0 else F32(0))
                        gi = dy[i, f] if v > 0 else F32(0)
                        assert R.same_bits(g[i, f], gi)
                        rstd = F32(1) / np.sqrt(var[f] + F32(eps))
                        xhat = (x[i, f] - mean[f]) * rstd
                        inv_n = F32(1) / F32(16)
                        gm = F32(1) if gamma is None else gamma[f]
                        t = gi - dbeta[f] * inv_n
                        t = t - (xhat * dgamma[f]) * inv_n
                        assert R.same_bits(dx[i, f], (gm * rstd) * t)
                        q = gi if gamma is None else gi * gamma[f]
                        assert R.same_bits(dq[i, f], q / sd)
    # ReLU only and mask only
    x = R.exact_case(5, 8)["x"] * np.where(np.arange(8) % 2 == 0, F32(1), F32(0))     # with +0 and -0 inputs
    assert R.same_bits(R.bn_fwd_ref(x), np.where(x > 0, x, F32(0)))
    assert R.same_bits(R.bn_bwd_apply_ref(x, R.masked(x + F32(1), x > 0), None, None, None, None, None, 5), np.where(x > 0, x + F32(1), F32(0)))


def test_exact_data_has_the_relu_edge():
    """The exact data has forward values +0 and -0, both outcomes of the mask, and whole columns below zero."""
    c = R.exact_case(65, 64)
    v = R.bn_fwd_ref(c["x"], c["mean"], c["var"], c["gamma"], c["beta"], c["eps"], relu=False)
    assert ((v == 0) & ~np.signbit(v)).any() and ((v == 0) & np.signbit(v)).any()
    assert (v > 0).any() and (v < 0).any() and (v < 0).all(0).any()
    v = R.bn_fwd_ref(c["x"], c["mean"], c["var"], c["gamma"], None, c["eps"], relu=False)
    assert ((v == 0) & np.signbit(v)).any()
    assert np.array_equal(v.astype(np.float64), ((c["x"].astype(np.float64) - c["mean"]) / np.sqrt(c["var"].astype(np.float64))) * c["gamma"])


@pytest.mark.parametrize("cell", R.cells(), ids=R.cell_id)
def test_exact_inputs_meet_the_condition(cell):
    """For every shape of tests/test_gpu_norm.py every reduction input of the exact data -- x, (x - mean)^2, g, g * xhat for the mask of every pointer mode -- meets
    sum|term| / quantum < 2^24, and the restated float32 terms ARE the exact terms."""
    F, _, n, _ = cell
    c = R.exact_case(n, F)
    x, dy, mean, var, eps = c["x"], c["dy"], c["mean"], c["var"], c["eps"]
    R.check_exact(x)
    R.check_exact(R.sqdev_terms(x, mean))
    assert np.array_equal(R.sqdev_terms(x, mean), (x.astype(np.float64) - mean) ** 2)
    for mask in (None, R.relu_mask_ref(x, None, mean, var, c["gamma"], c["beta"], eps), R.relu_mask_ref(x, None, mean, var, None, None, eps)):
        t0, t1 = R.bn_bwd_terms(x, R.masked(dy, mask), mean, var, eps)
        R.check_exact(t0)
        R.check_exact(t1)
        g64 = dy.astype(np.float64) * (1.0 if mask is None else mask)
        assert np.array_equal(t1, g64 * (x.astype(np.float64) - mean) / np.sqrt(var.astype(np.float64)))


def test_largest_row_count_by_arithmetic():
    """The bounds the condition rests on, for n = MAX_ROWS: |x| <= 2 and |g| <= 2 on quantum 1; (x - mean)^2 <= 9 and
    |g * xhat| <= 2 * 3 * 2 = 12 on quantum 0.25."""
    n = R.MAX_ROWS
    assert max(c[2] for c in R.cells()) == n
    assert 2 * n < 2 ** 24 and 9 * n / 0.25 < 2 ** 24 and 12 * n / 0.25 < 2 ** 24


@pytest.mark.parametrize("n", [1, 2, 64])
def test_variance_is_exact_at_power_of_two_counts(n):
    """n in {1, 2, 64}: the mean of integers is a multiple of 1/64, (x - mean)^2 a multiple of 2^-12 that float32 holds, and the
    sum meets the condition: the biased variance has an exact float32 value."""
    x = R.exact_case(n, 33)["x"]
    mean = R.bn_stats_mean_ref(x)
    assert np.array_equal(mean.astype(np.float64), x.astype(np.float64).mean(0))
    var = R.exact_colsum(R.sqdev_terms(x, mean), 2.0 ** -12, scale=1.0 / n)
    assert np.array_equal(var.astype(np.float64), x.astype(np.float64).var(0))


def test_shuffling_rows_changes_no_bit_and_a_lost_row_changes_every_column():
    c = R.exact_case(1025, 12)
    x, dy, mean, var = c["x"], c["dy"], c["mean"], c["var"]
    perm = np.random.default_rng(5).permutation(len(x))
    t0, t1 = R.bn_bwd_terms(x, dy, mean, var, 0.0)
    for k, t in enumerate((x, t0, R.sqdev_terms(x, mean), t1)):
        ref = R.exact_colsum(t)
        assert np.array_equal(ref, R.exact_colsum(t[perm]))
        # a sequential float32 sum in two orders: both exact
        for order in (np.arange(len(t)), perm):
            acc = np.zeros(t.shape[1], dtype=np.float32)
            for i in order:
                acc = acc + t[i].astype(np.float32)
            assert np.array_equal(acc, ref)
        # dropping or doubling row i moves column f by t[i, f]: every column of x and g, and every column with mean = +-0.5 of the
        # two centred sums (where mean = +-1 a term is zero when x == mean: those columns are there for the ReLU edge)
        nz = (t != 0).all(0)
        assert nz.all() if k < 2 else np.array_equal(nz, np.abs(mean) == 0.5)
        s = t.sum(0, dtype=np.float64)
        assert ((s - t).astype(np.float32) != ref)[:, nz].all() and ((s + t).astype(np.float32) != ref)[:, nz].all()


def test_swapped_association_changes_bits():
    """gamma * (rstd * (...)) instead of (gamma * rstd) * (...): 34.2 % of the elements of this random case change (recorded
    when the test was written; any share above zero lets the GPU comparison fail on such a kernel)."""
    c = R.random_case(300, 64, seed=4)
    dgamma, dbeta = c["dy"][:64].sum(0), c["dy"][64:128].sum(0)
    args = (c["x"], c["dy"], c["mean"], c["var"], c["gamma"], dgamma, dbeta, 300, c["eps"])
    a, b = R.bn_bwd_apply_ref(*args), R.bn_bwd_apply_swapped(*args)
    share = float((R.bits(a) != R.bits(b)).mean())
    print(f"swapped association: {100 * share:.1f} % of the elements differ")
    assert share > 0.0
    assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()      # yet far inside the old rtol = 1e-4 bar


def test_rounding_bound_tells_the_one_pass_variance_apart():
    """The n <= 300 rounding leg: the two-pass variance in float32 sits inside gamma_(n+3) * sum|term| / n of the float64 value on
    the same float32 mean; E[x^2] - mean^2 in float32 on data with a large mean does not."""
    n, F = 300, 16
    x = (np.random.default_rng(6).uniform(-1, 1, (n, F)) + 30.0).astype(np.float32)
    inv_n = F32(1) / F32(n)
    acc = np.zeros(F, dtype=np.float32)
    for i in range(n):
        acc = acc + x[i]
    mean = acc * inv_n
    d = x - mean
    acc = np.zeros(F, dtype=np.float32)
    for i in range(n):
        acc = acc + d[i] * d[i]
    var = acc * inv_n
    terms = (x.astype(np.float64) - mean.astype(np.float64)) ** 2
    bound = R.gamma_k(n + 3) * terms.sum(0) / n
    assert (np.abs(var - terms.sum(0) / n) <= bound).all()
    acc = np.zeros(F, dtype=np.float32)
    for i in range(n):
        acc = acc + x[i] * x[i]
    one_pass = acc * inv_n - mean * mean
    assert (np.abs(one_pass - terms.sum(0) / n) > bound).all()
