"""CPU tests of tests/elementwise_ref.py, the restatement tests/test_gpu_elementwise.py holds the streaming kernels to: each
vectorised expression against plain loops, the exact inputs against the exactness condition at every shape the GPU file uses, and
proofs that the GPU comparisons can fail (beta as a flag, a lost row, a lost column)."""
import numpy as np
import pytest

from tests import elementwise_ref as E
from tests import norm_ref as R

F32 = np.float32


def test_colsum_inputs_meet_the_condition_for_every_shape():
    """Every (F, n) of the GPU file's colsum grid (400 003 x 4 included) and of its rows_to_slots grid, every beta: `colsum_ref`
    asserts 2 n + |beta * out| / 0.125 < 2^24 quanta per column, and its result is the float64 sum."""
    shapes = [(n, F, 0) for F, _, n, _ in E.COLSUM_CASES] + [(n, F, 1) for F in E.SLOT_WIDTHS for n in E.SLOT_ROWS]
    for n, F, seed in sorted(set(shapes)):
        G, out = E.exact_matrix(n, F, seed), E.exact_out(F)
        s = G.sum(0, dtype=np.float64)
        for beta in E.BETAS:
            ref = E.colsum_ref(G, beta, None if beta == 0 else out)
            assert np.array_equal(ref.astype(np.float64), beta * out.astype(np.float64) * (beta != 0) + s)
    assert 2 * 400_003 / E.OUT_QUANTUM + 16 / E.OUT_QUANTUM < 2 ** 24


def test_colsum_reference_against_loops_and_beta_as_a_flag():
    G, out = E.exact_matrix(37, 9), E.exact_out(9)
    for beta in E.BETAS:
        ref = E.colsum_ref(G, beta, None if beta == 0 else out)
        for f in range(9):
            acc = F32(0)
            for i in range(37):
                acc = acc + G[i, f]
            assert ref[f] == (F32(beta) * out[f] + acc if beta != 0 else acc)
        flag = E.colsum_beta_as_flag(G, beta, out)
        # the old kernel (beta != 0 taken as 1) is told apart at 0.5 and -2 in every column, and agrees at 0 and 1
        assert np.array_equal(flag, ref) if beta in (0.0, 1.0) else (flag != ref).all()
    # beta == 0 does not read out
    assert np.array_equal(E.colsum_ref(G, 0.0, np.full(9, np.nan, dtype=np.float32)), E.colsum_ref(G, 0.0, None))
    # no rows: beta * out
    assert np.array_equal(E.colsum_ref(G[:0], 0.5, out), F32(0.5) * out) and not E.colsum_ref(G[:0], 0.0).any()


def test_a_lost_row_or_column_changes_every_sum():
    G = E.exact_matrix(129, 12)
    ref, s = E.colsum_ref(G), G.sum(0, dtype=np.float64)
    assert np.array_equal(ref, E.colsum_ref(G[np.random.default_rng(1).permutation(129)]))
    assert ((s - G).astype(np.float32) != ref).all() and ((s + G).astype(np.float32) != ref).all()
    rs = E.rowsum_exact_ref(G)
    assert ((G.sum(1, dtype=np.float64)[:, None] - G).astype(np.float32) != rs[:, None]).all()


@pytest.mark.parametrize("C", E.ROWSUM_COLS)
def test_rowsum_references(C):
    X = E.exact_matrix(9, C, seed=3)
    assert np.array_equal(E.rowsum_exact_ref(X), E.rowsum_ascending_ref(X))       # exact data: any order
    Xr = np.random.default_rng(C).uniform(-1, 1, (5, C)).astype(np.float32)
    got = E.rowsum_ascending_ref(Xr)
    for r in range(5):
        acc = F32(0)
        for c in range(C):
            acc = acc + Xr[r, c]
        assert R.same_bits(got[r], acc)


def test_small_ops_against_loops():
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-1, 1, 50).astype(np.float32), rng.uniform(-1, 1, 50).astype(np.float32)
    a, lr, wd = 0.3, 0.01, 5e-4
    ax, s1, s0 = E.axpy_ref(a, x, y), E.sgd_ref(y, x, lr, wd), E.sgd_ref(y, x, lr, 0.0)
    for i in range(50):
        assert R.same_bits(ax[i], y[i] + F32(a) * x[i])
        assert R.same_bits(s1[i], y[i] - F32(lr) * (x[i] + F32(wd) * y[i]))
        assert R.same_bits(s0[i], y[i] - F32(lr) * x[i])
    # the roundings are where they are said to be: a fused or reassociated form differs somewhere on 10^5 elements
    x, y = rng.uniform(-1, 1, 100_000).astype(np.float32), rng.uniform(-1, 1, 100_000).astype(np.float32)
    fused = (y.astype(np.float64) + np.float64(F32(a)) * x.astype(np.float64)).astype(np.float32)
    assert (R.bits(E.axpy_ref(a, x, y)) != R.bits(fused)).any()
    other = f32_sgd_distributed(y, x, lr, wd)
    assert (R.bits(E.sgd_ref(y, x, lr, wd)) != R.bits(other)).any()
    # wd == 0 skips the add: an infinite parameter makes no NaN gradient term
    assert np.isinf(E.sgd_ref(np.array([np.inf], dtype=np.float32), np.array([1.0], dtype=np.float32), 0.1, 0.0)[0])


def f32_sgd_distributed(p, g, lr, wd):
    """(p - lr * g) - (lr * wd) * p: equal in exact arithmetic, not in float32."""
    return (p - F32(lr) * g) - (F32(lr) * F32(wd)) * p


def test_gather_scatter_and_slots():
    X = E.exact_matrix(20, 5)
    idx = np.array([3, 3, 19, 0, 7], dtype=np.int32)
    assert np.array_equal(E.gather_ref(X, idx), np.stack([X[i] for i in idx]))
    Y, inp, uniq = E.exact_matrix(20, 5, seed=1), E.exact_matrix(4, 5, seed=2), np.array([9, 0, 19, 4], dtype=np.int32)
    got, loop = E.scatter_add_ref(Y, inp, uniq), Y.copy()
    for k, r in enumerate(uniq):
        loop[r] = loop[r] + inp[k]
    assert np.array_equal(got, loop)
    with pytest.raises(AssertionError):
        E.scatter_add_ref(Y, inp, np.array([1, 1, 2, 3]))
    for per_row in ((0,), (1,), (7,), (0, 1, 7, 0, 2)):
        send_idx = E.send_list(20, per_row)
        table = E.slot_table_ref(send_idx, 20)
        assert ((table >= 0).sum(1) == [per_row[r % len(per_row)] for r in range(20)]).all()
        for row in table:       # ascending, packed to the front
            k = int((row >= 0).sum())
            assert (row[:k] >= 0).all() and (np.diff(row[:k]) > 0).all() and (row[k:] == -1).all()
        send = E.rows_to_slots_ref(X, table, len(send_idx) + 2, -7.0)
        assert np.array_equal(send[:len(send_idx)], E.gather_ref(X, send_idx)) and (send[len(send_idx):] == -7.0).all()


def test_bf16_table():
    """The plain round-to-nearest-even restatement on the special values: the ties go to even in both directions, the largest finite
    float overflows to inf, denormals round among denormals, and torch.bfloat16 (the GPU test's reference) agrees."""
    import torch
    u = E.BF16_TABLE
    got = dict(zip(u.tolist(), E.bf16_rne_ref(u).tolist()))
    assert got[0x3F808000] == 0x3F80 and got[0x3F818000] == 0x3F82 and got[0x3F808001] == 0x3F81 and got[0x3F807FFF] == 0x3F80
    assert got[0xBF808000] == 0xBF80 and got[0xBF818000] == 0xBF82
    assert got[0x7F7FFFFF] == 0x7F80 and got[0xFF7FFFFF] == 0xFF80 and got[0x7F7F7FFF] == 0x7F7F and got[0x7F7F8000] == 0x7F80
    assert got[0x00000001] == 0x0000 and got[0x80000001] == 0x8000 and got[0x00008000] == 0x0000 and got[0x00018000] == 0x0002
    assert got[0x007FFFFF] == 0x0080 and got[0x80000000] == 0x8000
    t = torch.from_numpy(u.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(t, E.bf16_rne_ref(u))
    n = torch.from_numpy(E.BF16_NANS.view(np.int32).copy()).view(torch.float32)
    assert bool(torch.isnan(n).all()) and bool(torch.isnan(n.to(torch.bfloat16).float()).all())
