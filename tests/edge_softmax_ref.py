"""NumPy restatements of the edge softmax (gnnx_edge_softmax_csr_f32, gnnx_edge_softmax_bwd_csr_f32; include/gnnx.h "edge softmax")
and the patterns its tests share (tests/test_edge_softmax_cpu.py, tests/test_gpu_edge_softmax.py, tests/test_gpu_gat.py).

Independent of the kernels: plain float32 ufuncs in the header's order, every operation rounded on its own (NumPy's float32 ufuncs
round each operation; nothing is fused).  The row sum is the header's ROW ORDER -- G = min(64, pow2 >= d) virtual lanes for a row of
d <= S = 4096 entries, lane l adding entries l, l + G, ... ascending from +0, then the xor butterfly s = 1 .. G / 2; a longer row
in segments of S entries, each with G = 64, added in ascending segment order.  The one step that is NOT restated bit for bit is
expf: the GPU tests take the device's own x = expf(e - m) (the unnormalised output), hold it to float64 exp of the same float32
argument in ulps, and restate everything around it -- the maximum, the row sum, the division, the whole backward -- exactly."""
import numpy as np

S = 4096   # the contract's segment length

# row lengths of pattern A: every G from 1 to 64 with and without idle lanes, two to four entries per lane, the last length of one
# segment, the first of two, a whole second segment, three segments and a short fourth
LENGTHS_A = (0, 1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 12293)
N_COLS_A = 16384


def lanes_of(d):
    """G of a row (or segment) of d <= S entries: the smallest power of two >= d, capped at 64."""
    G = 1
    while G < d and G < 64:
        G *= 2
    return G


def row_of_entries(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr))


def _sum_lanes(V, G):
    """float32 [m]: the sums of the rows of float32 [m, d], d <= S, over G virtual lanes and the butterfly."""
    m, d = V.shape
    acc = np.zeros((m, G), dtype=np.float32)               # lane l starts from +0; a lane with no entry keeps it
    lanes = np.arange(G)
    for j in range(-(-d // G)):                            # entry k = l + j G of lane l, ascending
        k = lanes + j * G
        have = k < d
        acc[:, have] = acc[:, have] + V[:, k[have]]
    s = 1
    while s < G:                                           # acc_l = acc_l + acc_{l xor s}
        acc = acc + acc[:, lanes ^ s]
        s *= 2
    assert acc.dtype == np.float32
    return acc[:, 0].copy()


def sum_equal_rows(V):
    """float32 [m]: the sums of m rows of one length d (float32 [m, d]) in the row order."""
    V = np.ascontiguousarray(V, dtype=np.float32)
    m, d = V.shape
    if d <= S:
        return _sum_lanes(V, lanes_of(d))
    total = _sum_lanes(V[:, :S], 64)
    for s0 in range(S, d, S):                              # ((seg_0 + seg_1) + seg_2) + ...
        total = total + _sum_lanes(V[:, s0:s0 + S], 64)
    assert total.dtype == np.float32
    return total


def row_sum_in_order(v, rowptr):
    """float32 [n_rows]: the row sums of the per-entry values v (float32 [nnz]) in the row order; an empty row gives +0."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    deg = np.diff(rowptr)
    out = np.zeros(deg.shape[0], dtype=np.float32)
    for d in np.unique(deg):
        if d == 0:
            continue
        rows = np.nonzero(deg == d)[0]
        idx = rowptr[rows][:, None] + np.arange(d)[None, :]
        out[rows] = sum_equal_rows(v[idx])
    return out


def sum_ascending(V):
    """The plain order: one accumulator, entries ascending (what the row order must be told apart from).  float32 [m] of [m, d]."""
    return np.cumsum(np.ascontiguousarray(V, dtype=np.float32), axis=1, dtype=np.float32)[:, -1].copy()


def pre_activation(rowptr, colidx, scores=None, rowterm=None, colterm=None):
    """float32 [nnz]: t_p = (scores[p] + rowterm[i]) + colterm[c_p], a None operand skipped."""
    f32 = lambda a: None if a is None else np.asarray(a, dtype=np.float32)  # noqa: E731
    scores, rowterm, colterm = f32(scores), f32(rowterm), f32(colterm)
    assert scores is not None or rowterm is not None or colterm is not None
    rows, cols = row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    t = None
    for term in (scores, None if rowterm is None else rowterm[rows], None if colterm is None else colterm[cols]):
        if term is not None:
            t = term.copy() if t is None else t + term
    assert t.dtype == np.float32
    return t


def leaky(t, slope):
    t = np.asarray(t, dtype=np.float32)
    return np.where(t > 0, t, t * np.float32(slope)).astype(np.float32)


def row_max(e, rowptr):
    """float32 [n_rows]: the maximum of each row's entries, -inf on an empty row."""
    m = np.full(len(rowptr) - 1, -np.inf, dtype=np.float32)
    np.maximum.at(m, row_of_entries(rowptr), np.asarray(e, dtype=np.float32))
    return m


def exp_argument(e, rowptr):
    """(float32 [nnz] e_p - m_i rounded once, float32 [n_rows] m): what the device hands to expf."""
    m = row_max(e, rowptr)
    return (np.asarray(e, dtype=np.float32) - m[row_of_entries(rowptr)]).astype(np.float32), m


def edge_softmax_from_x(x, z, rowptr):
    """float32 [nnz]: alpha_p = x_p / z_i, one IEEE division."""
    out = np.asarray(x, dtype=np.float32) / np.asarray(z, dtype=np.float32)[row_of_entries(rowptr)]
    assert out.dtype == np.float32
    return out


def edge_softmax_ref(rowptr, colidx, scores=None, rowterm=None, colterm=None, slope=1.0):
    """(alpha, x, m, z) in float32 with NumPy's own float32 exp: the whole forward in the contract's order, up to the exp's last bit."""
    e = leaky(pre_activation(rowptr, colidx, scores, rowterm, colterm), slope)
    arg, m = exp_argument(e, rowptr)
    x = np.exp(arg).astype(np.float32)
    z = row_sum_in_order(x, rowptr)
    return edge_softmax_from_x(x, z, rowptr), x, m, z


def edge_softmax_bwd_ref(rowptr, colidx, alpha, dalpha, scores=None, rowterm=None, colterm=None, slope=1.0):
    """(dt float32 [nnz], drowterm float32 [n_rows]) bit for bit: w = alpha * dalpha; dot = row sum of w; de = alpha * (dalpha - dot);
    dt = t > 0 ? de : de * slope; drowterm = row sum of dt."""
    alpha, dalpha = np.asarray(alpha, dtype=np.float32), np.asarray(dalpha, dtype=np.float32)
    rows = row_of_entries(rowptr)
    t = pre_activation(rowptr, colidx, scores, rowterm, colterm)
    dot = row_sum_in_order(alpha * dalpha, rowptr)
    de = alpha * (dalpha - dot[rows])
    dt = np.where(t > 0, de, de * np.float32(slope)).astype(np.float32)
    return dt, row_sum_in_order(dt, rowptr)


def edge_softmax_ref64(rowptr, colidx, n_cols, scores=None, rowterm=None, colterm=None, slope=1.0, dalpha=None):
    """float64 model of the float32 inputs: dict(alpha) and, with dalpha, dt (= dL/dscores), drowterm, dcolterm and absum =
    sum_p |alpha_p dalpha_p| per row (the condition of the backward's row sums)."""
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)  # noqa: E731
    rows, cols = row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    n_rows = len(rowptr) - 1
    t = np.zeros(len(cols))
    if scores is not None:
        t = t + f64(scores)
    if rowterm is not None:
        t = t + f64(rowterm)[rows]
    if colterm is not None:
        t = t + f64(colterm)[cols]
    e = np.where(t > 0, t, t * float(np.float32(slope)))
    m = np.full(n_rows, -np.inf)
    np.maximum.at(m, rows, e)
    x = np.exp(e - m[rows])
    z = np.bincount(rows, weights=x, minlength=n_rows)
    alpha = x / z[rows]
    out = dict(alpha=alpha, e=e, m=m, z=z)
    if dalpha is not None:
        w = alpha * f64(dalpha)
        dot = np.bincount(rows, weights=w, minlength=n_rows)
        de = alpha * (f64(dalpha) - dot[rows])
        dt = np.where(t > 0, de, de * float(np.float32(slope)))
        out.update(dt=dt, drowterm=np.bincount(rows, weights=dt, minlength=n_rows), dcolterm=np.bincount(cols, weights=dt, minlength=n_cols),
                   absum=np.bincount(rows, weights=np.abs(w), minlength=n_rows))
    return out


def pattern_a(seed=7):
    """Pattern A: (rowptr int32, colidx int32, lengths) over N_COLS_A columns.  One row of every length of LENGTHS_A plus runs of short
    and empty rows, shuffled so that the hubs sit between them; the first and the last row are empty.  Columns ascending, no repeats."""
    rng = np.random.default_rng(seed)
    lengths = list(LENGTHS_A) + [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 5, 7, 11, 13, 16, 17] * 3
    lengths = [0] + [int(d) for d in rng.permutation(lengths)] + [0]
    cols = [np.sort(rng.choice(N_COLS_A, d, replace=False)) for d in lengths]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return rowptr, np.concatenate(cols).astype(np.int32), np.array(lengths)


def chain_bound(d):
    """The row order's error bound in units of 2^-24 * sum |v|: the longest chain of additions an entry goes through --
    ceil(min(d, S) / G) in its lane, log2 G in the butterfly, ceil(d / S) over the segments."""
    G = lanes_of(min(d, S)) if d <= S else 64
    return -(-min(d, S) // G) + int(np.log2(G)) + -(-d // S)
