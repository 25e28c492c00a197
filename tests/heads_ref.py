"""NumPy restatements of the multi-head calls (gnnx_spmm_csr_heads_f32, gnnx_sddmm_csr_heads_f32, gnnx_edge_softmax_csr_heads_f32,
gnnx_edge_softmax_bwd_csr_heads_f32; include/gnnx.h "multi-head attention") for tests/test_heads_cpu.py, tests/test_gpu_heads.py and
tests/test_gpu_gat_heads.py.

Direct restatements, all heads at once: float32 ufuncs in the header's orders, every operation rounded on its own.  Feature matrices are
[rows, H * D] with head h in columns h D .. h D + D - 1; per-entry arrays are entry-major [nnz, H].  The aggregation keeps ONE accumulator
per output element and takes a row's entries from its last position down (tests/spmm_ref.py's walk with a value per entry and head); the
scores are tests/sddmm_ref.py's dots_in_lane_order on the [entries * H, D] slabs (the lane-group order with F := D); the softmax sums
every (row, head) with tests/edge_softmax_ref.py's sum_equal_rows (the ROW ORDER).  tests/test_heads_cpu.py shows each of them equal to
the loop of single-head restatements over the heads, bit for bit."""
import numpy as np

from tests import edge_softmax_ref as er
from tests import sddmm_ref as sr

CELLS_CPU = ((8, 8), (4, 6), (3, 5), (8, 1), (2, 64))   # (H, D) of the CPU comparison


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def spmm_heads_ref(rowptr, colidx, X, vals, n_heads, bias=None, y0=None, relu_out=False):
    """float32 [n_rows, H D]: Y[i, h D + j] = relu?(y0 + ((sum_p vals[p, h] * X[c_p, h D + j]) + bias)), a row's entries taken from its
    last position down: t = X[c_p] * vals[p, head]; acc = acc + t.  y0 is the beta = 1 form."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    X, vals, bias, y0 = _f32(X), _f32(vals), _f32(bias), _f32(y0)
    H = int(n_heads)
    n_rows, F = rowptr.shape[0] - 1, X.shape[1]
    assert F % H == 0 and vals.shape == (colidx.shape[0], H)
    D = F // H
    deg, end = np.diff(rowptr), rowptr[1:]
    order = np.argsort(-deg, kind="stable")          # longest rows first: the rows of step k are a prefix
    sorted_deg = deg[order]
    acc = np.zeros((n_rows, H, D), dtype=np.float32)
    for k in range(int(deg.max()) if n_rows else 0):
        rows = order[:int(np.searchsorted(-sorted_deg, -k, side="left"))]   # degree > k
        p = end[rows] - 1 - k
        t = X[colidx[p]].reshape(-1, H, D) * vals[p][:, :, None]
        acc[rows] = acc[rows] + t
    acc = acc.reshape(n_rows, F)
    if bias is not None:
        acc = acc + bias[None, :]
    if y0 is not None:
        acc = y0 + acc
    if relu_out:
        acc = np.where(acc > 0, acc, np.float32(0))
    assert acc.dtype == np.float32
    return acc


def sddmm_heads_ref(rowptr, colidx, L, R, n_heads):
    """float32 [nnz, H]: out[p, h] = <L[i, slab h], R[c_p, slab h]> in the lane-group order of F = D."""
    L, R = _f32(L), _f32(R)
    H = int(n_heads)
    F = R.shape[1]
    assert F % H == 0 and L.shape[1] == F
    D = F // H
    rows, cols = sr.row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    nnz = cols.shape[0]
    out = np.zeros((nnz, H), dtype=np.float32)
    for p0 in range(0, nnz, sr.ENTRY_BLOCK):
        sl = slice(p0, min(nnz, p0 + sr.ENTRY_BLOCK))
        out[sl] = sr.dots_in_lane_order(L[rows[sl]].reshape(-1, D), R[cols[sl]].reshape(-1, D)).reshape(-1, H)
    return out


def pre_activation_heads(rowptr, colidx, scores=None, rowterm=None, colterm=None):
    """float32 [nnz, H]: t[p, h] = (scores[p, h] + rowterm[i, h]) + colterm[c_p, h], a None operand skipped."""
    scores, rowterm, colterm = _f32(scores), _f32(rowterm), _f32(colterm)
    assert scores is not None or rowterm is not None or colterm is not None
    rows, cols = er.row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    t = None
    for term in (scores, None if rowterm is None else rowterm[rows], None if colterm is None else colterm[cols]):
        if term is not None:
            t = term.copy() if t is None else t + term
    assert t.dtype == np.float32 and t.ndim == 2
    return t


def row_sum_in_order_heads(v, rowptr):
    """float32 [n_rows, H]: the sums over each row's entries of v (float32 [nnz, H]) in the row order, per head; an empty row gives +0."""
    v = _f32(v)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    H = v.shape[1]
    deg = np.diff(rowptr)
    out = np.zeros((deg.shape[0], H), dtype=np.float32)
    for d in np.unique(deg):
        if d == 0:
            continue
        rows = np.nonzero(deg == d)[0]
        idx = rowptr[rows][:, None] + np.arange(d)[None, :]
        V = v[idx].transpose(0, 2, 1).reshape(-1, d)         # one line per (row, head)
        out[rows] = er.sum_equal_rows(V).reshape(-1, H)
    return out


def row_max_heads(e, rowptr):
    """float32 [n_rows, H]: the maximum of each row's entries per head, -inf on an empty row."""
    e = _f32(e)
    m = np.full((len(rowptr) - 1, e.shape[1]), -np.inf, dtype=np.float32)
    np.maximum.at(m, er.row_of_entries(rowptr), e)
    return m


def exp_argument_heads(e, rowptr):
    """(float32 [nnz, H] e - m rounded once, float32 [n_rows, H] m): what the device hands to expf."""
    m = row_max_heads(e, rowptr)
    return (_f32(e) - m[er.row_of_entries(rowptr)]).astype(np.float32), m


def edge_softmax_heads_from_x(x, z, rowptr):
    """float32 [nnz, H]: alpha = x / z[row], one IEEE division."""
    out = _f32(x) / _f32(z)[er.row_of_entries(rowptr)]
    assert out.dtype == np.float32
    return out


def edge_softmax_heads_ref(rowptr, colidx, scores=None, rowterm=None, colterm=None, slope=1.0):
    """(alpha, x, m, z) in float32 with NumPy's own float32 exp: the whole forward in the contract's order, up to the exp's last bit."""
    e = er.leaky(pre_activation_heads(rowptr, colidx, scores, rowterm, colterm), slope)
    arg, m = exp_argument_heads(e, rowptr)
    x = np.exp(arg).astype(np.float32)
    z = row_sum_in_order_heads(x, rowptr)
    return edge_softmax_heads_from_x(x, z, rowptr), x, m, z


def edge_softmax_heads_bwd_ref(rowptr, colidx, alpha, dalpha, scores=None, rowterm=None, colterm=None, slope=1.0):
    """(dt float32 [nnz, H], drowterm float32 [n_rows, H]) bit for bit: w = alpha * dalpha; dot = row sum of w; de = alpha * (dalpha - dot);
    dt = t > 0 ? de : de * slope; drowterm = row sum of dt."""
    alpha, dalpha = _f32(alpha), _f32(dalpha)
    rows = er.row_of_entries(rowptr)
    t = pre_activation_heads(rowptr, colidx, scores, rowterm, colterm)
    dot = row_sum_in_order_heads(alpha * dalpha, rowptr)
    de = alpha * (dalpha - dot[rows])
    dt = np.where(t > 0, de, de * np.float32(slope)).astype(np.float32)
    return dt, row_sum_in_order_heads(dt, rowptr)


def slab(M, h, n_heads):
    """Column slab h of a [rows, H D] matrix, contiguous."""
    D = M.shape[1] // n_heads
    return np.ascontiguousarray(M[:, h * D:(h + 1) * D])
