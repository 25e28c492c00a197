"""A NumPy float32 restatement of the neighbourhood reductions (gnnx_spmm_csr_reduce_f32 / gnnx_spmm_csr_reduce_bwd_f32,
include/gnnx.h "neighbourhood reductions"), independent of the kernels: the forward's first-occurrence arg-max / arg-min per row, the
backward's routed sum in the header's order -- segments of S entries, each ONE accumulator from +0 walking from the segment's last
entry to its first, the segment sums added in ascending order; every multiply and add separately rounded (NumPy's float32 ufuncs
round each operation; nothing is fused).  tests/test_reduce_cpu.py pins both to plain loops, to float64 autograd and to
tests/spmm_ref.py."""
import numpy as np

SEG = 4096   # S of the contract


def transpose_csr(rowptr, colidx, n_cols):
    """(rowptr_t, colidx_t, map_t) of a CSR with ascending columns and no duplicates: row c of CSR(A^T) lists the rows that store
    column c, ascending; map_t[q] is the position in CSR(A) of entry q of CSR(A^T) (what gnnx_csr_transpose_map finds)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(colidx, kind="stable")
    rowptr_t = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(colidx, minlength=n_cols), out=rowptr_t[1:])
    return rowptr_t.astype(np.int32), rows[order].astype(np.int32), order.astype(np.int32)


def spmm_reduce_ref(rowptr, colidx, X, vals=None, op="max"):
    """(Y float32 [n_rows, F], arg int32 [n_rows, F]): per row T = vals[:, None] * X[cols] in float32 (X[cols] itself without vals),
    arg = the first occurrence of the column's maximum (minimum) as an absolute position, Y = T[arg].  Empty rows: +0 and -1."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    X = np.ascontiguousarray(X, dtype=np.float32)
    T = X[colidx]
    if vals is not None:
        T = np.ascontiguousarray(vals, dtype=np.float32)[:, None] * T
    assert T.dtype == np.float32
    pick = {"max": np.argmax, "min": np.argmin}[op]
    n_rows, F = len(rowptr) - 1, X.shape[1]
    Y = np.zeros((n_rows, F), dtype=np.float32)
    arg = np.full((n_rows, F), -1, dtype=np.int32)
    cols = np.arange(F)
    for i in range(n_rows):
        b, e = rowptr[i], rowptr[i + 1]
        if e > b:
            a = pick(T[b:e], axis=0)      # the first occurrence
            Y[i] = T[b:e][a, cols]
            arg[i] = b + a
    return Y, arg


def spmm_reduce_bwd_ref(rowptr_t, colidx_t, map_t, arg, G, vals=None, y0=None, S=SEG):
    """dX float32 [n_rows_t, F] = (y0 +) the routed sum: entry q of row c of CSR(A^T), with i = colidx_t[q] and p = map_t[q], adds
    vals[p] * G[i, f] (rounded; G[i, f] without vals) where arg[i, f] == p.  Row c is cut into segments of S entries; a segment is one
    accumulator per feature from +0 over its entries LAST to FIRST; the row is ((seg_0 + seg_1) + seg_2) + ...  Vectorised over the
    segments by position from the top: step k touches the segments with more than k entries."""
    rowptr_t = np.asarray(rowptr_t, dtype=np.int64)
    colidx_t = np.asarray(colidx_t, dtype=np.int64)
    map_t = np.asarray(map_t, dtype=np.int64)
    arg = np.asarray(arg, dtype=np.int64)
    G = np.ascontiguousarray(G, dtype=np.float32)
    vals = None if vals is None else np.ascontiguousarray(vals, dtype=np.float32)
    n_rows, F = len(rowptr_t) - 1, G.shape[1]
    deg = np.diff(rowptr_t)
    nseg = -(-deg // S)
    first = np.concatenate([[0], np.cumsum(nseg)])                 # a row's first segment
    seg_row = np.repeat(np.arange(n_rows), nseg)
    seg_k = np.arange(first[-1]) - first[seg_row]                  # the segment's number inside its row
    seg_b = rowptr_t[seg_row] + seg_k * S
    seg_e = np.minimum(seg_b + S, rowptr_t[seg_row + 1])
    seg_len = seg_e - seg_b
    order = np.argsort(-seg_len, kind="stable")                    # longest first: the segments of step k are a prefix
    sorted_len = seg_len[order]
    part = np.zeros((len(seg_row), F), dtype=np.float32)
    for k in range(int(seg_len.max()) if len(seg_len) else 0):
        segs = order[:int(np.searchsorted(-sorted_len, -k, side="left"))]   # more than k entries
        q = seg_e[segs] - 1 - k
        i, p = colidx_t[q], map_t[q]
        t = G[i]
        if vals is not None:
            t = vals[p][:, None] * t
        part[segs] = np.where(arg[i] == p[:, None], part[segs] + t, part[segs])
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
