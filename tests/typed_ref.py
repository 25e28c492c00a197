"""A NumPy float32 restatement of the relation-typed aggregation (gnnx_spmm_csr_typed_f32 / gnnx_spmm_csr_typed_bwd_f32 /
gnnx_typed_coeff_grad_f32, include/gnnx.h "relation-typed aggregation"), independent of the kernels: one rounding per operation (NumPy's
float32 ufuncs round each; nothing is fused) and the header's order as loops -- segments of S entries, each ONE accumulator per output
element from +0 walking from the segment's last entry to its first, the segment sums added in ascending order; in one-hot mode an
entry of another type is absent from a slab's chain (a select, never an add of zero)."""
import numpy as np

from tests.pool_ref import pool_fwd
from tests.sddmm_ref import ENTRY_BLOCK, dots_in_lane_order, row_of_entries

SEG = 4096   # S of the contract


def _row_sums(rowptr, terms, shape, S):
    """float32 [n_rows, *shape]: terms(q) -> (t [len(q), *shape], take or None) for the entry positions q; an accumulator adds t where
    take holds (everywhere without one).  Vectorised over the segments by position from the top: step k touches the segments with more
    than k entries."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n_rows = len(rowptr) - 1
    nseg = -(-np.diff(rowptr) // S)
    first = np.concatenate([[0], np.cumsum(nseg)])                 # a row's first segment
    seg_row = np.repeat(np.arange(n_rows), nseg)
    seg_b = rowptr[seg_row] + (np.arange(first[-1]) - first[seg_row]) * S
    seg_e = np.minimum(seg_b + S, rowptr[seg_row + 1])
    order = np.argsort(-(seg_e - seg_b), kind="stable")            # longest first: the segments of step k are a prefix
    sorted_len = (seg_e - seg_b)[order]
    part = np.zeros((len(seg_row),) + shape, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(sorted_len[0]) if len(sorted_len) else 0):
            segs = order[:int(np.searchsorted(-sorted_len, -k, side="left"))]   # more than k entries
            t, take = terms(seg_e[segs] - 1 - k)
            assert t.dtype == np.float32
            part[segs] = part[segs] + t if take is None else np.where(take, part[segs] + t, part[segs])
        acc = np.zeros((n_rows,) + shape, dtype=np.float32)
        have = np.nonzero(nseg > 0)[0]
        acc[have] = part[first[have]]
        for j in range(1, int(nseg.max()) if n_rows else 0):
            rows = np.nonzero(nseg > j)[0]
            acc[rows] = acc[rows] + part[first[rows] + j]
    return acc


def _weights(C, etype, vals, q):
    """w [len(q), B]: C[t_p, b] * v_p, one rounding; C[t_p, b] itself without vals."""
    w = C[etype[q]]
    return w if vals is None else w * vals[q][:, None]


def spmm_typed_ref(rowptr, colidx, etype, X, n_types, C=None, vals=None, S=SEG):
    """M float32 [n_rows, B F]; C None is one-hot mode (B = n_types)."""
    colidx, etype = np.asarray(colidx, dtype=np.int64), np.asarray(etype, dtype=np.int64)
    B, F = (n_types if C is None else C.shape[1]), X.shape[1]

    def terms(q):
        x = X[colidx[q]]
        if C is None:
            m = x if vals is None else x * vals[q][:, None]
            return np.broadcast_to(m[:, None, :], (len(q), B, F)), (etype[q][:, None] == np.arange(B))[:, :, None]
        return _weights(C, etype, vals, q)[:, :, None] * x[:, None, :], None

    return _row_sums(rowptr, terms, (B, F), S).reshape(len(rowptr) - 1, B * F)


def spmm_typed_bwd_ref(rowptr_t, colidx_t, etype_t, dM, n_types, F, C=None, vals_t=None, y0=None, S=SEG):
    """dX float32 [n_rows_t, F] = (y0 +) the row sums of u_q on the transposed pattern: the slab terms chained in ascending b."""
    colidx_t, etype_t = np.asarray(colidx_t, dtype=np.int64), np.asarray(etype_t, dtype=np.int64)
    B = n_types if C is None else C.shape[1]

    def terms(q):
        g = dM[colidx_t[q]].reshape(len(q), B, F)
        if C is None:
            u = g[np.arange(len(q)), etype_t[q]]
            return (u if vals_t is None else u * vals_t[q][:, None]), None
        w = _weights(C, etype_t, vals_t, q)
        u = w[:, 0, None] * g[:, 0]
        for b in range(1, B):
            u = u + w[:, b, None] * g[:, b]
        return u, None

    acc = _row_sums(rowptr_t, terms, (F,), S)
    return acc if y0 is None else np.ascontiguousarray(y0, dtype=np.float32) + acc


def typed_coeff_grad_ref(rowptr, colidx, etype, dM, X, n_types, n_slabs, vals=None):
    """(dC float32 [R, B], D float32 [nnz, B]): the per-entry slab dots in the lane-group order of tests/sddmm_ref.py, v_p applied
    last, then each type's rows of D summed in the order of the segment readout (tests/pool_ref.py) over the type-sorted entries."""
    rows, cols, etype = row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64), np.asarray(etype, dtype=np.int64)
    F = X.shape[1]
    D = np.zeros((len(cols), n_slabs), dtype=np.float32)
    for p0 in range(0, len(cols), ENTRY_BLOCK):
        sl = slice(p0, min(len(cols), p0 + ENTRY_BLOCK))
        for b in range(n_slabs):
            d = dots_in_lane_order(dM[rows[sl], b * F:(b + 1) * F], X[cols[sl]])
            D[sl, b] = d if vals is None else d * vals[sl]
    order = np.argsort(etype, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(etype, minlength=n_types))]).astype(np.int32)
    return pool_fwd(ptr, D[order], "sum")[0], D
