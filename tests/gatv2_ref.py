"""NumPy restatements of the dynamic-attention calls (gnnx_gatv2_scores_csr_f32, gnnx_gatv2_scores_bwd_csr_f32; include/gnnx.h "dynamic
attention scores (GATv2)") for tests/test_gatv2_ref_cpu.py, tests/test_gpu_gatv2.py and tests/test_gpu_gatv2_stack.py.

Plain float32 ufuncs in the header's orders, one rounding per operation (NumPy's float32 ufuncs round each operation; nothing is fused).
Feature matrices are [rows, H * D] with head h in columns h D .. h D + D - 1; per-entry arrays are entry-major [nnz, H].
  scores_ref      u = L[i] + R[c]; e = u > 0 ? u : u * slope; term = a * e; the sum over a head's D terms by tests/sddmm_ref.py's
                  dots_in_lane_order (the lane-group order with F := D: its product a * e IS the term, rounded before the add).
  scores_bwd_ref  one accumulator per (row, feature) from +0, a Python loop over the row's entries from its last position down:
                  w = u > 0 ? a : a * slope (rounded once); acc = acc + de[m, h] * w; T likewise with e in the place of w.
  *_ref64         the same formulas in float64 with plain sums: what the float32 results are near, and what they EQUAL on the exact family.
  exact_case      the exact family: L, R from {-2 .. 2}, a from {-1, -.5, 0, .5, 1}, de from {-1, 0, 1}, slope 0.5.  Every u, e, w and term
                  is a multiple of 2^-2 and, by the asserted bound sum |term| / 2^-2 < 2^24 for every output, so is every partial sum in
                  any order: each operation is exact and every result has the bits of the float64 sum.  u == 0 occurs on purpose (it
                  takes the slope branch)."""
import numpy as np

from tests import sddmm_ref as sr

EXACT_SLOPE = 0.5
QUANTUM = 2.0 ** -2


# the dynamic-attention case: rows 0 and 1 both store columns A = 0 and B = 1; row 0 scores A above B, row 1 B above A (slope 0.2)
DYNAMIC = dict(pattern=(np.array([0, 2, 4], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32)),
               L=np.array([[0, 0], [-3, 1]], dtype=np.float32), R=np.array([[2, -2], [0, 0]], dtype=np.float32),
               a=np.array([1, 1], dtype=np.float32))


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _pattern(rowptr, colidx):
    return np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)


def make_pattern(seed, n_rows, n_cols):
    """(rowptr int32, colidx int32), ascending columns without duplicates: degrees 0 .. 11 (empty rows; several rows inside one group of 32
    entries; rows that end inside one), row 3 with 65 and row 17 with 300 entries (each longer than a 64-wide window); nnz is odd."""
    rng = np.random.default_rng(seed)
    deg = rng.choice([0, 0, 1, 2, 3, 5, 7, 11], n_rows)
    deg[3], deg[17] = 65, 300
    if deg.sum() % 2 == 0:
        deg[5] += 1
    assert deg.max() <= n_cols and (deg == 0).any() and deg.sum() % 32 and deg.sum() % 4
    colidx = np.concatenate([np.sort(rng.choice(n_cols, d, replace=False)) for d in deg])
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), colidx.astype(np.int32)


def leaky32(u, slope):
    out = np.where(u > 0, u, u * np.float32(slope))
    assert out.dtype == np.float32
    return out


def scores_ref(rowptr, colidx, L, R, a, n_heads, slope):
    """float32 [nnz, H]: the GATv2 score of every stored entry in the lane-group order of F = D."""
    L, R, a = _f32(L), _f32(R), _f32(a)
    H = int(n_heads)
    F = R.shape[1]
    assert F % H == 0 and L.shape[1] == F and a.shape == (F,)
    D = F // H
    rows, cols = sr.row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    nnz = cols.shape[0]
    out = np.zeros((nnz, H), dtype=np.float32)
    for p0 in range(0, nnz, sr.ENTRY_BLOCK):
        sl = slice(p0, min(nnz, p0 + sr.ENTRY_BLOCK))
        e = leaky32(L[rows[sl]] + R[cols[sl]], slope)                        # u rounded, then the slope product
        A = np.broadcast_to(a, e.shape)
        out[sl] = sr.dots_in_lane_order(A.reshape(-1, D), e.reshape(-1, D)).reshape(-1, H)
    assert out.dtype == np.float32
    return out


def scores_ref64(rowptr, colidx, L, R, a, n_heads, slope):
    L, R, a = (np.asarray(x, dtype=np.float64) for x in (L, R, a))
    H = int(n_heads)
    rows, cols = sr.row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    u = L[rows] + R[cols]
    e = np.where(u > 0, u, u * float(slope))
    return (a[None, :] * e).reshape(len(cols), H, -1).sum(axis=2)


def scores_bwd_ref(rowptr, colidx, de, own, other, a, n_heads, slope, entry_map=None, y0=None, want_T=False):
    """(dOwn, T) float32 [n_rows, H D] (T None without want_T).  y0 is the beta = 1 form: dOwn = y0 + acc."""
    rowptr, colidx = _pattern(rowptr, colidx)
    de, own, other, a, y0 = _f32(de), _f32(own), _f32(other), _f32(a), _f32(y0)
    H = int(n_heads)
    n_rows, F = own.shape
    assert F % H == 0 and other.shape[1] == F and a.shape == (F,) and de.shape == (colidx.shape[0], H)
    D = F // H
    m = np.arange(colidx.shape[0], dtype=np.int64) if entry_map is None else np.asarray(entry_map, dtype=np.int64)
    a_slope = a * np.float32(slope)                                          # rounded once
    acc = np.zeros((n_rows, F), dtype=np.float32)
    tacc = np.zeros((n_rows, F), dtype=np.float32)
    for i in range(n_rows):
        for p in range(int(rowptr[i + 1]) - 1, int(rowptr[i]) - 1, -1):      # descending stored position
            u = own[i] + other[colidx[p]]
            d = np.repeat(de[m[p]], D)                                       # the entry's gradient of the feature's head
            w = np.where(u > 0, a, a_slope)
            acc[i] = acc[i] + d * w
            if want_T:
                tacc[i] = tacc[i] + d * leaky32(u, slope)
    if y0 is not None:
        acc = y0 + acc
    assert acc.dtype == np.float32 and tacc.dtype == np.float32
    return acc, (tacc if want_T else None)


def scores_bwd_ref64(rowptr, colidx, de, own, other, a, n_heads, slope, entry_map=None):
    """(dOwn, T, da) in float64 with plain sums; da = the column sums of T = the gradient of a."""
    rowptr, colidx = _pattern(rowptr, colidx)
    de, own, other, a = (np.asarray(x, dtype=np.float64) for x in (de, own, other, a))
    H = int(n_heads)
    n_rows, F = own.shape
    D = F // H
    rows = sr.row_of_entries(rowptr)
    if entry_map is not None:
        de = de[np.asarray(entry_map, dtype=np.int64)]
    u = own[rows] + other[colidx]
    d = np.repeat(de, D, axis=1)
    dOwn, T = np.zeros((n_rows, F)), np.zeros((n_rows, F))
    np.add.at(dOwn, rows, d * np.where(u > 0, a[None, :], a[None, :] * float(slope)))
    np.add.at(T, rows, d * np.where(u > 0, u, u * float(slope)))
    return dOwn, T, T.sum(axis=0)


def _assert_exact(terms, index, n_out):
    """terms: float64 [nnz, k], the terms of the outputs [index[p], j].  Every term is a multiple of 2^-2 and sum |term| / 2^-2 < 2^24 for
    every output: every partial sum in any order is then a multiple of 2^-2 of fewer than 24 bits -- a float32."""
    terms = np.asarray(terms, dtype=np.float64)
    assert np.array_equal(terms / QUANTUM, np.round(terms / QUANTUM)), "a term is not a multiple of 2^-2"
    total = np.zeros((n_out, terms.shape[1]))
    np.add.at(total, index, np.abs(terms))
    assert (total / QUANTUM < 2.0 ** 24).all()


def exact_case(seed, rowptr, colidx, n_cols, n_heads, head_dim):
    """dict(L, R, a, de, slope) of the exact family on a pattern, with the module's bound asserted for out, dOwn, T and colsum(T) (and
    for dR on any pattern with the same entries: its terms are those of dOwn, grouped by column)."""
    rowptr, colidx = _pattern(rowptr, colidx)
    rng = np.random.default_rng(seed)
    n_rows, nnz, H, D = rowptr.shape[0] - 1, colidx.shape[0], int(n_heads), int(head_dim)
    F = H * D
    L = rng.integers(-2, 3, (n_rows, F)).astype(np.float32)
    R = rng.integers(-2, 3, (n_cols, F)).astype(np.float32)
    a = (rng.integers(-2, 3, F) * 0.5).astype(np.float32)
    de = rng.integers(-1, 2, (nnz, H)).astype(np.float32)
    rows = sr.row_of_entries(rowptr)
    u = L[rows].astype(np.float64) + R[colidx]
    e = np.where(u > 0, u, u * EXACT_SLOPE)
    assert (u == 0).any() or nnz == 0, "the family is meant to hold exact zeros of u"
    d = np.repeat(de.astype(np.float64), D, axis=1)
    w = np.where(u > 0, a[None, :].astype(np.float64), a[None, :] * EXACT_SLOPE)
    # out[p, h]: the D terms a * e of entry p and head h -- one line of D terms per output, no two outputs share one
    _assert_exact((a[None, :] * e).reshape(nnz * H, D).T, np.zeros(D, dtype=np.int64), 1)
    _assert_exact(d * w, rows, n_rows)                                       # dOwn
    _assert_exact(d * w, colidx, n_cols)                                     # dR on the transposed pattern
    _assert_exact(d * e, rows, n_rows)                                       # T
    _assert_exact(d * e, np.zeros(nnz, dtype=np.int64), 1)                   # colsum(T)
    return dict(L=L, R=R, a=a, de=de, slope=EXACT_SLOPE)
