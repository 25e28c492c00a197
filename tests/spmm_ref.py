"""A NumPy restatement of the aggregation (gnnx_spmm_csr_f32 and its fused / bf16 variants, include/gnnx.h), the documented
kernel dispatch as a five-line rule, and the width lists of the dispatch tests (tests/test_spmm_ref_cpu.py,
tests/test_gpu_spmm_dispatch.py).

spmm_ref is independent of the kernels and of the C oracle: plain float32 elementwise arithmetic in the header's order --
per row ONE accumulator per feature starting from zero, neighbours taken from the row's last position down (descending column),
every multiply and add separately rounded (NumPy's float32 ufuncs round each operation; nothing is fused).  It is pinned to
oracle/gcn_oracle.c bit for bit and to float64 within the suite's condition-aware bar by tests/test_spmm_ref_cpu.py."""
import numpy as np

# ---- widths of the GPU dispatch tests: each list is proved to cover the dispatch table by tests/test_spmm_ref_cpu.py ----
VEC4_WIDTHS = (4, 12, 16, 20, 24, 32, 36, 48, 64, 68, 72, 128, 132, 256, 260, 516)   # aligned f32 rows, 16-byte pieces
VEC1_WIDTHS = (1, 3, 5, 7, 9, 13, 15, 17, 21, 31, 33, 63, 65, 101, 130, 257)         # aligned f32 rows, scalar lanes
UNALIGNED_WIDTHS = (4, 8, 16, 32, 64, 128, 256)   # multiples of 4 placed so that one vec4 condition fails: the scalar-lane fallback
BF16_UNALIGNED_WIDTHS = (32, 100, 128)      # bf16 rows that are not 8-byte aligned


def spmm_cell(F, aligned=True):
    """(VEC, G, kernel, tiles) of a call of width F as gnnx_spmm.hip's spmm_impl documents its choice; aligned: every pointer and
    leading dimension meets the vec4 conditions.  Used to prove coverage of the table, never as a second implementation."""
    vec = 4 if aligned and F % 4 == 0 else 1
    lanes = F // vec
    G = 64 if lanes > 32 else 32 if lanes > 16 else 16 if lanes > 8 else 8 if lanes > 4 else 4
    return vec, G, "stream" if G >= 32 else "rows", -(-F // (G * vec))


def spmm_ref(rowptr, colidx, X, vals=None, colscale=None, rowscale=None, bias=None, y0=None, relu_out=False):
    """Y = relu?(y0 + (rowscale (.) sum_p vals[p] * colscale[c_p] * X[c_p, :] + bias)) as float32 [n_rows, F].
    Per neighbour p of a row, last position first: t = X[c_p]; t = t * colscale[c_p]; t = t * vals[p]; acc = acc + t.  After the row:
    acc * rowscale[row], + bias, y0 + acc (the beta = 1 form), where(acc > 0, acc, 0).  Vectorised over rows by position from the
    top: step k touches the rows with more than k entries."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    X, vals, colscale, rowscale, bias, y0 = f32(X), f32(vals), f32(colscale), f32(rowscale), f32(bias), f32(y0)
    n_rows = rowptr.shape[0] - 1
    deg = np.diff(rowptr)
    end = rowptr[1:]
    order = np.argsort(-deg, kind="stable")          # longest rows first: the rows of step k are a prefix
    sorted_deg = deg[order]
    acc = np.zeros((n_rows, X.shape[1]), dtype=np.float32)
    for k in range(int(deg.max()) if n_rows else 0):
        rows = order[:int(np.searchsorted(-sorted_deg, -k, side="left"))]   # degree > k
        p = end[rows] - 1 - k
        c = colidx[p]
        t = X[c]
        if colscale is not None:
            t = t * colscale[c][:, None]
        if vals is not None:
            t = t * vals[p][:, None]
        acc[rows] = acc[rows] + t
    if rowscale is not None:
        acc = acc * rowscale[:, None]
    if bias is not None:
        acc = acc + bias[None, :]
    if y0 is not None:
        acc = y0 + acc
    if relu_out:
        acc = np.where(acc > 0, acc, np.float32(0))
    assert acc.dtype == np.float32
    return acc
