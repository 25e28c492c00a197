"""Pure-numpy restatement of the receptive-field sets and blocks (include/gnnx.h, "query inference"): the yardstick of
tests/test_gpu_receptive.py, itself held to hand-written expectations by tests/test_receptive_cpu.py.

With Q_L = the unique ascending query rows and Q_{l-1} = the set of columns stored in rows Q_l of the CSR, layer l's block is the
CSR of rows Q_l with every column replaced by its position in Q_{l-1}, entries in stored order."""
import numpy as np


def ref_frontier(rowptr, colidx, rows):
    """(ascending unique columns stored in the listed rows, number of entries of the listed rows)"""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    parts = [colidx[rowptr[r]:rowptr[r + 1]] for r in np.asarray(rows, dtype=np.int64)]
    ent = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return np.unique(ent).astype(np.int32), int(ent.size)


def ref_extract(rowptr, colidx, rows, col_set=None, vals=None):
    """(rowptr', colidx', vals' or None) of the listed rows; col_set (ascending unique): columns become positions in it, and a
    column outside it raises KeyError."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    lens = rowptr[rows + 1] - rowptr[rows] if rows.size else np.zeros(0, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    src = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows]).astype(np.int64) if rows.size else np.zeros(0, dtype=np.int64)
    ci = colidx[src]
    if col_set is not None:
        col_set = np.asarray(col_set, dtype=np.int64)
        p = np.searchsorted(col_set, ci)
        if ci.size and (col_set.size == 0 or np.any(p >= col_set.size) or np.any(col_set[np.minimum(p, col_set.size - 1)] != ci)):
            raise KeyError("a column of the listed rows is not in the set")
        ci = p
    return rp, ci.astype(np.int32), None if vals is None else np.asarray(vals)[src]


def ref_field(rowptr, colidx, query, L):
    """query: ROWS of the CSR, any order, repeats allowed.  -> dict(rows=[Q_0 .. Q_L], nnz=[0, nnz_1 .. nnz_L],
    blocks=[None, (rowptr', colidx')_1 .. _L], query_pos = position of every query entry in Q_L)."""
    query = np.asarray(query, dtype=np.int64).reshape(-1)
    rows = [None] * (L + 1)
    rows[L] = np.unique(query).astype(np.int32)
    nnz, blocks = [0] * (L + 1), [None] * (L + 1)
    for l in range(L, 0, -1):
        rows[l - 1], nnz[l] = ref_frontier(rowptr, colidx, rows[l])
        rp, ci, _ = ref_extract(rowptr, colidx, rows[l], col_set=rows[l - 1])
        blocks[l] = (rp, ci)
    return dict(rows=rows, nnz=nnz, blocks=blocks, query_pos=np.searchsorted(rows[L], query).astype(np.int32))
