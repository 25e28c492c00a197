"""A NumPy float32 restatement of the edge-feature aggregation (gnnx_spmm_csr_edge_f32 / gnnx_spmm_csr_edge_bwd_f32, include/gnnx.h
"edge features"), independent of the kernels: one rounding per operation (NumPy's float32 ufuncs round each; nothing is fused) and the
header's order as loops -- segments of S entries, each ONE accumulator from +0 walking from the segment's last entry to its first, the
segment sums added in ascending order."""
import numpy as np

SEG = 4096   # S of the contract


def messages(X, E, cols, rows_e, msg):
    """t of the entries whose columns and edge rows are given: act(X[c] + E[e]) (act(E[e]) without X) in float32."""
    m = E[rows_e] if X is None else X[cols] + E[rows_e]
    assert m.dtype == np.float32
    return np.where(m > 0, m, np.float32(0)) if msg == "relu" else m       # NaN and -0 become +0


def spmm_edge_ref(rowptr, colidx, X, E, eidx=None, msg="relu", y0=None, S=SEG):
    """Y float32 [n_rows, F] = (y0 +) the row sums.  Vectorised over the segments by position from the top: step k touches the
    segments with more than k entries."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    eidx = np.arange(len(colidx)) if eidx is None else np.asarray(eidx, dtype=np.int64)
    n_rows, F = len(rowptr) - 1, E.shape[1]
    nseg = -(-np.diff(rowptr) // S)
    first = np.concatenate([[0], np.cumsum(nseg)])                 # a row's first segment
    seg_row = np.repeat(np.arange(n_rows), nseg)
    seg_b = rowptr[seg_row] + (np.arange(first[-1]) - first[seg_row]) * S
    seg_e = np.minimum(seg_b + S, rowptr[seg_row + 1])
    order = np.argsort(-(seg_e - seg_b), kind="stable")            # longest first: the segments of step k are a prefix
    sorted_len = (seg_e - seg_b)[order]
    part = np.zeros((len(seg_row), F), dtype=np.float32)
    for k in range(int(sorted_len[0]) if len(sorted_len) else 0):
        segs = order[:int(np.searchsorted(-sorted_len, -k, side="left"))]   # more than k entries
        q = seg_e[segs] - 1 - k
        part[segs] = part[segs] + messages(X, E, colidx[q], eidx[q], msg)
    acc = np.zeros((n_rows, F), dtype=np.float32)
    have = np.nonzero(nseg > 0)[0]
    acc[have] = part[first[have]]
    for j in range(1, int(nseg.max()) if n_rows else 0):
        rows = np.nonzero(nseg > j)[0]
        acc[rows] = acc[rows] + part[first[rows] + j]
    if y0 is not None:
        acc = np.ascontiguousarray(y0, dtype=np.float32) + acc
    assert acc.dtype == np.float32
    return acc


def spmm_edge_bwd_ref(rowptr, colidx, X, E, G, eidx=None, msg="relu", fill=None):
    """dE float32 [edge rows, F]: row eidx[p] = G[i] where the message of entry p of row i was positive (relu) or G[i] (add); the rows
    that no entry names keep `fill` (zeros without one)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    eidx = np.arange(len(colidx)) if eidx is None else np.asarray(eidx, dtype=np.int64)
    g = G[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))]
    dE = np.zeros((E.shape[0], G.shape[1]), dtype=np.float32) if fill is None else fill.copy()
    if msg == "relu":
        m = E[eidx] if X is None else X[colidx] + E[eidx]
        g = np.where(m > 0, g, np.float32(0))
    dE[eidx] = g
    return dE
