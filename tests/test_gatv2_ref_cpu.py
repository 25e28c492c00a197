"""CPU tests of tests/gatv2_ref.py, the NumPy restatement that tests/test_gpu_gatv2.py holds the GATv2 kernels to: hand-written literals
and hand-written float32 chains on a 3-row pattern, equality with float64 on the exact family, the dynamic-attention property that the
score exists for and its converse for the GAT score, and da = colsum(T)."""
import itertools

import numpy as np
import pytest

from tests import gatv2_ref as gr
from tests import sddmm_ref as sr

f = np.float32

# row 0 stores columns 0 and 2, row 1 is empty, row 2 stores column 1
ROWPTR = np.array([0, 2, 2, 3], dtype=np.int32)
COLIDX = np.array([0, 2, 1], dtype=np.int32)
ENTRIES = ((0, 0), (0, 2), (2, 1))

# H = 2; the D = 3 operands are the first three features of each head of the D = 5 ones
L5 = np.array([[1, -2, .5, 1, -1, 2, -1, 0, 0, 2], [9, 9, 9, 9, 9, 9, 9, 9, 9, 9], [-1, 1, 1, 2, 0, 0, -3, 2, -1, 1]], dtype=np.float32)
R5 = np.array([[1, 1, -1.5, -3, 2, -2, 1, 1, 1, -1], [1, -2, .5, 1, 1, 1, 1, -1, -1, -2], [-3, 2, .5, 1, -1, 1, -1, 2, 2, 1]], dtype=np.float32)
A5 = np.array([1, -1, 2, .5, -2, .5, 1, -2, 1, 4], dtype=np.float32)
DE = np.array([[1, -1], [2, .5], [-1, 2]], dtype=np.float32)


def operands(D):
    keep = np.concatenate([np.arange(D), 5 + np.arange(D)])
    return L5[:, keep].copy(), R5[:, keep].copy(), A5[keep].copy()


def test_scores_literals_slope_half():
    """Worked by hand; with slope 0.5 every operation is exact, so the literals do not depend on the order."""
    L, R, a = operands(3)
    # entry 0 (row 0, col 0): u = [2 -1 -1 | 0 0 1], e = [2 -.5 -.5 | 0 0 1], a e = [2 .5 -1 | 0 0 -2]
    # entry 1 (row 0, col 2): u = [-2 0 1 | 3 -2 2], e = [-1 0 1 | 3 -1 2], a e = [-1 0 2 | 1.5 -1 -4]
    # entry 2 (row 2, col 1): u = [0 -1 1.5 | 1 -2 1], e = [0 -.5 1.5 | 1 -1 1], a e = [0 .5 3 | .5 -1 -2]
    assert np.array_equal(gr.scores_ref(ROWPTR, COLIDX, L, R, a, 2, 0.5), np.array([[1.5, -2], [1, -3.5], [3.5, -2.5]], dtype=np.float32))
    L, R, a = operands(5)
    # entry 0: a e = [2 .5 -1 -.5 -2 | 0 0 -2 1 4];  entry 1: [-1 0 2 1 2 | 1.5 -1 -4 2 12];  entry 2: [0 .5 3 1.5 -2 | .5 -1 -2 -1 -2]
    assert np.array_equal(gr.scores_ref(ROWPTR, COLIDX, L, R, a, 2, 0.5), np.array([[-1, 3], [4, 10.5], [3, -5.5]], dtype=np.float32))


def term(a, l, r, slope):
    """One term in scalar float32, each operation written out: u = l + r; e = u > 0 ? u : u * slope; a * e."""
    u = f(l) + f(r)
    e = u if u > 0 else u * f(slope)
    return f(a) * e


@pytest.mark.parametrize("slope", [0.2, 0.5])
def test_scores_hand_chains(slope):
    """D = 3 is one chunk on one lane: ((t0 + t1) + t2) from +0.  D = 5 is two chunks on two lanes: lane 0 adds t0 .. t3, lane 1 holds
    t4, and the butterfly adds the two."""
    for D in (3, 5):
        L, R, a = operands(D)
        got = gr.scores_ref(ROWPTR, COLIDX, L, R, a, 2, slope)
        assert got.dtype == np.float32 and got.shape == (3, 2)
        for p, (i, c) in enumerate(ENTRIES):
            for h in range(2):
                t = [term(a[h * D + k], L[i, h * D + k], R[c, h * D + k], slope) for k in range(D)]
                if D == 3:
                    want = ((f(0) + t[0]) + t[1]) + t[2]
                else:
                    lane0 = (((f(0) + t[0]) + t[1]) + t[2]) + t[3]
                    lane1 = f(0) + t[4]
                    want = lane0 + lane1
                assert got[p, h] == want and type(want) is np.float32, (D, p, h)


def test_scores_bwd_literals_slope_half():
    L, R, a = operands(3)
    dOwn, T = gr.scores_bwd_ref(ROWPTR, COLIDX, DE, L, R, a, 2, 0.5, want_T=True)
    # row 0: entry 1 then entry 0.  w1 = [.5 -.5 2 | .5 .5 -2], d1 = [2 | .5]: [1 -1 4 | .25 .25 -1];  w0 = [1 -.5 1 | .25 .5 -2], d0 = [1 | -1]:
    # [1 -.5 1 | -.25 -.5 2].  T: d1 e1 = [-2 0 2 | 1.5 -.5 1], d0 e0 = [2 -.5 -.5 | 0 0 -1].  row 2: w = [.5 -.5 2 | .5 .5 -2], d = [-1 | 2]
    assert np.array_equal(dOwn, np.array([[2, -1.5, 5, 0, -.25, 1], [0] * 6, [-.5, .5, -2, 1, 1, -4]], dtype=np.float32))
    assert np.array_equal(T, np.array([[0, -.5, 1.5, 1.5, -.5, 0], [0] * 6, [0, .5, -1.5, 2, -2, 2]], dtype=np.float32))
    y0 = np.full((3, 6), 10, dtype=np.float32)
    assert np.array_equal(gr.scores_bwd_ref(ROWPTR, COLIDX, DE, L, R, a, 2, 0.5, y0=y0)[0], y0 + dOwn)   # beta = 1; exact here
    assert gr.scores_bwd_ref(ROWPTR, COLIDX, DE, L, R, a, 2, 0.5)[1] is None


@pytest.mark.parametrize("slope", [0.2, 0.5])
@pytest.mark.parametrize("D", [3, 5])
def test_scores_bwd_hand_chains(D, slope):
    """Row 0 in scalar float32: from +0, entry 1 first, then entry 0; w's slope product rounded once."""
    L, R, a = operands(D)
    dOwn, T = gr.scores_bwd_ref(ROWPTR, COLIDX, DE, L, R, a, 2, slope, want_T=True)
    for j in range(2 * D):
        h = j // D
        acc, tacc = f(0), f(0)
        for p in (1, 0):
            u = L[0, j] + R[COLIDX[p], j]
            w = a[j] if u > 0 else a[j] * f(slope)
            e = u if u > 0 else u * f(slope)
            acc = acc + DE[p, h] * w
            tacc = tacc + DE[p, h] * e
        assert dOwn[0, j] == acc and T[0, j] == tacc and type(acc) is np.float32
    assert not dOwn[1].any() and not T[1].any()   # the empty row


def patterns():
    """(rowptr, colidx, n_cols): the 3-row pattern, and a seeded one with empty rows, a row of 65 and one of 300 entries."""
    rp, ci = gr.make_pattern(5, 40, 320)
    return [(ROWPTR, COLIDX, 3), (rp, ci, 320)]


@pytest.mark.parametrize("H,D", [(1, 1), (2, 3), (3, 5), (2, 16), (1, 260)])
def test_exact_family_equals_float64(H, D):
    for k, (rp, ci, n_cols) in enumerate(patterns()):
        if k == 0 and H * D < 4:
            continue   # too few (entry, feature) pairs for the family's exact zeros of u
        case = gr.exact_case(100 + k, rp, ci, n_cols, H, D)
        L, R, a, de, slope = (case[x] for x in ("L", "R", "a", "de", "slope"))
        out = gr.scores_ref(rp, ci, L, R, a, H, slope)
        assert np.array_equal(out.astype(np.float64), gr.scores_ref64(rp, ci, L, R, a, H, slope))
        dOwn, T = gr.scores_bwd_ref(rp, ci, de, L, R, a, H, slope, want_T=True)
        dOwn64, T64, da64 = gr.scores_bwd_ref64(rp, ci, de, L, R, a, H, slope)
        assert np.array_equal(dOwn.astype(np.float64), dOwn64) and np.array_equal(T.astype(np.float64), T64)
        # da from T: the column sums of the restated T are the float64 gradient of a (any order: exact)
        da = np.zeros(H * D, dtype=np.float32)
        for i in range(T.shape[0]):
            da = da + T[i]
        assert np.array_equal(da.astype(np.float64), da64)
        # the column side on the transposed pattern: de stays in the forward order and is reached through the map
        rp_t, ci_t = sr.transpose_csr(rp, ci, n_cols)
        map_t = sr.transpose_map_ref(rp, ci, rp_t, ci_t)
        dR, none = gr.scores_bwd_ref(rp_t, ci_t, de, R, L, a, H, slope, entry_map=map_t)
        assert none is None
        dR_by_hand, _ = gr.scores_bwd_ref(rp_t, ci_t, de[map_t], R, L, a, H, slope)
        assert np.array_equal(dR, dR_by_hand)
        rows = sr.row_of_entries(rp)
        u = L[rows].astype(np.float64) + R[ci]
        dR64 = np.zeros(R.shape)
        np.add.at(dR64, ci, np.repeat(de.astype(np.float64), D, axis=1) * np.where(u > 0, a[None, :], a[None, :].astype(np.float64) * slope))
        assert np.array_equal(dR.astype(np.float64), dR64)


def test_gradients_match_float64_autograd():
    """The three gradients (dL, dR, da) of sum(out * de) against torch's float64 autograd of the same formula."""
    torch = pytest.importorskip("torch")
    rp, ci, n_cols = patterns()[1]
    H, D, slope = 3, 5, 0.2
    rng = np.random.default_rng(7)
    L = rng.standard_normal((len(rp) - 1, H * D)).astype(np.float32)
    R = rng.standard_normal((n_cols, H * D)).astype(np.float32)
    a = rng.standard_normal(H * D).astype(np.float32)
    de = rng.standard_normal((len(ci), H)).astype(np.float32)
    tl, tr, ta = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (L, R, a))
    rows = torch.from_numpy(sr.row_of_entries(rp))
    cols = torch.from_numpy(ci.astype(np.int64))
    e = (ta * torch.nn.functional.leaky_relu(tl[rows] + tr[cols], float(f(slope)))).view(len(ci), H, D).sum(2)
    (e * torch.from_numpy(de.astype(np.float64))).sum().backward()
    assert np.abs(gr.scores_ref(rp, ci, L, R, a, H, slope) - e.detach().numpy()).max() <= 1e-5
    dL, T = gr.scores_bwd_ref(rp, ci, de, L, R, a, H, slope, want_T=True)
    rp_t, ci_t = sr.transpose_csr(rp, ci, n_cols)
    dR, _ = gr.scores_bwd_ref(rp_t, ci_t, de, R, L, a, H, slope, entry_map=sr.transpose_map_ref(rp, ci, rp_t, ci_t))
    for got, ref in ((dL, tl.grad), (dR, tr.grad), (T.astype(np.float64).sum(0), ta.grad)):
        ref = ref.numpy()
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


def test_dynamic_attention_two_rows_rank_the_same_columns_in_opposite_order():
    """Rows 0 and 1 both store columns A = 0 and B = 1.  With a = [1, 1], R_A = [2, -2], R_B = [0, 0] and slope 0.2:
    row 0, L = [0, 0]:   e(A) = 2 + 0.2 * -2 = 1.6;            e(B) = 0                       -> A above B
    row 1, L = [-3, 1]:  e(A) = 0.2 * -1 + 0.2 * -1 = -0.4;    e(B) = 0.2 * -3 + 1 = 0.4       -> B above A."""
    e = gr.scores_ref(*gr.DYNAMIC["pattern"], gr.DYNAMIC["L"], gr.DYNAMIC["R"], gr.DYNAMIC["a"], 1, 0.2).reshape(2, 2)
    assert e[0, 0] > e[0, 1] and e[1, 1] > e[1, 0]
    assert np.allclose(e, [[1.6, 0], [-0.4, 0.4]], rtol=1e-6, atol=0)


def test_argument_errors_need_no_device():
    """Validation comes before any device call: the statuses come back on a machine without a GPU; nnz == 0 is OK with no launch."""
    import importlib

    import __graft_entry__ as ge
    ge.build()
    lib = importlib.import_module("gnncpp_amd.capi").lib()
    fwd, bwd = lib.gnnx_gatv2_scores_csr_f32, lib.gnnx_gatv2_scores_bwd_csr_f32
    assert fwd(4, 4, 2, 8, 0, None, None, None, 16, None, 16, None, 0.2, None, 2, None) == 0
    assert bwd(0, 4, 2, 8, 0, None, None, None, 2, None, None, 16, None, 16, None, 0.2, 0.0, None, 16, None, 16, None) == 0
    for args in ((-1, 4, 2, 8, 0, None, None, None, 16, None, 16, None, 0.2, None, 2, None),
                 (4, 4, 0, 8, 0, None, None, None, 16, None, 16, None, 0.2, None, 2, None),
                 (4, 4, 2, 0, 0, None, None, None, 16, None, 16, None, 0.2, None, 2, None),
                 (4, 4, 2, 8, 1 << 31, None, None, None, 16, None, 16, None, 0.2, None, 2, None),
                 (4, 4, 2, 8, 0, None, None, None, 15, None, 16, None, 0.2, None, 2, None),
                 (4, 4, 2, 8, 0, None, None, None, 16, None, 16, None, 0.2, None, 1, None),
                 (4, 4, 2, 8, 3, None, None, None, 16, None, 16, None, 0.2, None, 2, None)):
        assert fwd(*args) == -1, args
    assert b"null" in lib.gnnx_last_error()
    for args in ((4, -1, 2, 8, 0, None, None, None, 2, None, None, 16, None, 16, None, 0.2, 0.0, None, 16, None, 16, None),
                 (4, 4, 2, 8, 0, None, None, None, 1, None, None, 16, None, 16, None, 0.2, 0.0, None, 16, None, 16, None),
                 (4, 4, 2, 8, 0, None, None, None, 2, None, None, 16, None, 16, None, 0.2, 0.5, None, 16, None, 16, None),
                 (4, 4, 2, 8, 0, None, None, None, 2, None, None, 16, None, 16, None, 0.2, 0.0, None, 15, None, 16, None),
                 (4, 4, 2, 8, 0, None, None, None, 2, None, None, 16, None, 16, None, 0.2, 0.0, None, 16, None, 16, None)):
        assert bwd(*args) == -1, args
    assert b"null" in lib.gnnx_last_error()


def test_gat_score_is_static():
    """The converse: leaky_relu is increasing and the row term is constant within a row, so leaky(el_i + er_c) ranks two columns by their
    er alone -- the same way in every row, whatever the terms."""
    grid = [-3.0, -1.0, -0.25, 0.0, 0.5, 2.0]
    leaky = lambda t, s: t if t > 0 else t * s  # noqa: E731
    for slope in (0.2, 0.5, 1.0):
        for el0, el1, er_a, er_b in itertools.product(grid, repeat=4):
            rank0 = np.sign(leaky(el0 + er_a, slope) - leaky(el0 + er_b, slope))
            rank1 = np.sign(leaky(el1 + er_a, slope) - leaky(el1 + er_b, slope))
            assert rank0 == rank1 == np.sign(er_a - er_b)
