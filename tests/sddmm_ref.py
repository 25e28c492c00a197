"""NumPy restatements of the edge-score entry points (gnnx_sddmm_csr_f32, gnnx_csr_transpose_map, gnnx_bce_logits_f32;
include/gnnx.h) and the width list of the GPU test (tests/test_sddmm_cpu.py, tests/test_gpu_sddmm.py, tests/test_gpu_link.py).

sddmm_ref is independent of the kernels: plain float32 ufuncs in the header's order -- Q = ceil(F / 4) chunks of four features,
G = min(64, pow2 >= Q) accumulators starting from +0, accumulator l takes chunks l, l + G, ... in ascending f with the product
rounded before the sum, then the xor butterfly s = 1, 2, ..., G / 2 -- every operation rounded on its own (NumPy's float32 ufuncs
round each operation; nothing is fused).  tests/test_sddmm_cpu.py holds it to float64 and shows that the order is visible in the
bits."""
import numpy as np

# every G from 1 to 64, idle lanes (Q < G), a ragged last chunk (F % 4 != 0), 2, 3 and 4 chunks per lane
WIDTHS = (1, 3, 4, 5, 8, 12, 16, 20, 32, 33, 64, 65, 100, 101, 128, 132, 256, 257, 260, 516, 1024)

ENTRY_BLOCK = 4096   # entries per vectorised step of sddmm_ref (bounds the [entries, F] temporaries)


def lane_group(F):
    """(Q, G, chunks per lane): Q = ceil(F / 4) chunks; G the smallest power of two >= Q, capped at 64."""
    Q = -(-int(F) // 4)
    G = 1
    while G < Q and G < 64:
        G *= 2
    return Q, G, -(-Q // G) if Q else 0


def row_of_entries(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr))


def dots_in_lane_order(A, B):
    """float32 [m]: <A[k,:], B[k,:]> of float32 [m, F] operands in the documented lane-group order."""
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    m, F = A.shape
    Q, G, cpl = lane_group(F)
    prod = A * B                                            # every product rounded to float32 first
    acc = np.zeros((m, G), dtype=np.float32)                # lane l starts from +0; a lane with no chunk keeps it
    lanes = np.arange(G)
    for c in range(cpl):                                    # chunk q = l + c G of lane l
        for j in range(4):                                  # ascending f inside the chunk
            f = 4 * (lanes + c * G) + j
            have = f < F
            acc[:, have] = acc[:, have] + prod[:, f[have]]
    s = 1
    while s < G:                                            # acc_l = acc_l + acc_{l xor s}
        acc = acc + acc[:, lanes ^ s]
        s *= 2
    assert acc.dtype == np.float32
    return acc[:, 0].copy()


def sddmm_ref(rowptr, colidx, L, R, rowscale=None, colscale=None):
    """float32 [nnz]: out[p] = (dot_p * rowscale[i]) * colscale[c_p], dot_p = <L[i,:], R[c_p,:]> in the lane-group order; each
    scale skipped when None, each multiply rounded on its own."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    L, R, rowscale, colscale = f32(L), f32(R), f32(rowscale), f32(colscale)
    rows = row_of_entries(rowptr)
    cols = np.asarray(colidx, dtype=np.int64)
    nnz = cols.shape[0]
    assert rows.shape[0] == nnz
    out = np.zeros(nnz, dtype=np.float32)
    for p0 in range(0, nnz, ENTRY_BLOCK):
        sl = slice(p0, min(nnz, p0 + ENTRY_BLOCK))
        d = dots_in_lane_order(L[rows[sl]], R[cols[sl]])
        if rowscale is not None:
            d = d * rowscale[rows[sl]]
        if colscale is not None:
            d = d * colscale[cols[sl]]
        out[sl] = d
    assert out.dtype == np.float32
    return out


def dots_ascending(A, B):
    """The plain order: one accumulator, f ascending (what the lane-group order must be told apart from)."""
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    prod = A * B
    acc = np.zeros(A.shape[0], dtype=np.float32)
    for f in range(A.shape[1]):
        acc = acc + prod[:, f]
    return acc


def transpose_map_ref(rowptr, colidx, rowptr_t, colidx_t):
    """int32 [nnz]: for entry q = (c, r) of CSR(A^T) the position of (r, c) in CSR(A); KeyError when it has none."""
    pos = {(int(r), int(c)): p for p, (r, c) in enumerate(zip(row_of_entries(rowptr), np.asarray(colidx)))}
    assert len(pos) == len(colidx), "duplicate entries"
    return np.array([pos[(int(r), int(c))] for c, r in zip(row_of_entries(rowptr_t), np.asarray(colidx_t))], dtype=np.int32)


def bce_logits_ref64(x, y, n_total=None):
    """float64 (loss, sigmoid(x) - y): loss = sum_p [log(1 + exp(x_p)) - x_p y_p] / n_total; the second is n_total * dscores."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n_total = x.size if n_total is None else n_total
    loss = float((np.logaddexp(0.0, x) - x * y).sum() / n_total)
    return loss, 1.0 / (1.0 + np.exp(-x)) - y


def random_csr(seed, n_rows, n_cols, nnz_target):
    """A seeded pattern with ascending columns and no duplicates: (rowptr int32, colidx int32)."""
    rng = np.random.default_rng(seed)
    key = np.unique(rng.integers(0, n_rows, nnz_target).astype(np.int64) * n_cols + rng.integers(0, n_cols, nnz_target))
    rows, cols = key // n_cols, key % n_cols
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols.astype(np.int32)


def transpose_csr(rowptr, colidx, n_cols):
    """CSR(A^T) of a pattern with ascending columns, ascending columns again: (rowptr_t, colidx_t)."""
    rows, cols = row_of_entries(rowptr), np.asarray(colidx, dtype=np.int64)
    order = np.lexsort((rows, cols))
    rowptr_t = np.zeros(n_cols + 1, dtype=np.int64)
    np.add.at(rowptr_t, cols + 1, 1)
    return np.cumsum(rowptr_t).astype(np.int32), rows[order].astype(np.int32)
