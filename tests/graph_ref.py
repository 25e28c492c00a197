"""A NumPy restatement of the graph build (gnn.cpp_amd/csrc/gnnx_graph.hip: gnnx_csr_from_coo, gnnx_csr_from_coo_weighted,
gnnx_degree_norm_f32, include/gnnx.h) and the case lists of tests/test_gpu_graph_build.py.

Independent of the kernels and of the C oracle: sorting is NumPy's stable argsort of one integer key per edge, the weighted
adjacency is also written as the reference defines it (a dense matrix assigned edge by edge in list order, then scanned row-major),
and the degree block is tests/spmm_ref.py's float32 sum at width 1.  tests/test_graph_ref_cpu.py pins all of it to
oracle/gcn_oracle.c and to the golden vectors of the compiled reference, and proves that the case lists below can tell a wrong
kernel from a right one.  Everything here is integer work or strictly ordered float32: every comparison against it is equality."""
import numpy as np

from tests.spmm_ref import spmm_ref

# flags and diagonal modes of include/gnnx.h
KEEP_SELF_LOOPS, KEEP_DUPLICATES, DROP_TRUNCATED_ZERO = 1, 2, 4
DIAG_KEEP, DIAG_STRIP, DIAG_FILL = 0, 1, 2
LONG_ROW = 128          # gnnx_graph.hip kLongRow: rows of at least this many entries are norm_long_kernel's


def _endpoints(src, dst, n):
    r = np.asarray(src, dtype=np.int64).reshape(-1)
    c = np.asarray(dst, dtype=np.int64).reshape(-1)
    assert r.shape == c.shape
    if r.size and (r.min() < 0 or c.min() < 0 or r.max() >= n or c.max() >= n):
        raise ValueError("invalid input, max value in edge_index should be less than the number of nodes from x")
    return r, c


def _rowptr(rows, n):
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)


def csr_from_coo_ref(src, dst, n, keep_self_loops=False, keep_duplicates=False):
    """(rowptr int64 [n + 1], colidx int32 [nnz]) of gnnx_csr_from_coo: drop r == c unless kept, stable sort by (r, c), collapse
    runs of equal pairs unless duplicates are kept.  ValueError on an endpoint outside [0, n)."""
    r, c = _endpoints(src, dst, n)
    if not keep_self_loops:
        keep = r != c
        r, c = r[keep], c[keep]
    order = np.argsort(r * n + c, kind="stable")
    r, c = r[order], c[order]
    if not keep_duplicates and r.size:
        head = np.concatenate([[True], (r[1:] != r[:-1]) | (c[1:] != c[:-1])])
        r, c = r[head], c[head]
    return _rowptr(r, n), c.astype(np.int32)


def dropped(v):
    """GNNX_CSR_DROP_TRUNCATED_ZERO without a cast: an entry is dropped iff -1 < w < 1 (NaN, +-inf and every |w| >= 1 stay)."""
    v = np.asarray(v, dtype=np.float32)
    return (v > np.float32(-1)) & (v < np.float32(1))


def csr_from_coo_weighted_dense_ref(src, dst, w, n, diag_mode=DIAG_KEEP, diag_value=0.0, drop_truncated_zero=False):
    """Form (a), keep_duplicates = False only: the reference's definition.  A dense `present` mask and a dense value matrix,
    assigned edge by edge in list order (a later edge overwrites an earlier one); DIAG_STRIP clears the diagonal, DIAG_FILL assigns
    every (i, i) after the list; then a row-major scan.  O(n^2) memory: n <= ~2000."""
    r, c = _endpoints(src, dst, n)
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    assert w.shape == r.shape
    present = np.zeros((n, n), dtype=bool)
    A = np.zeros((n, n), dtype=np.float32)
    for e in range(r.size):                   # literally in list order
        present[r[e], c[e]] = True
        A[r[e], c[e]] = w[e]
    d = np.arange(n)
    if diag_mode == DIAG_STRIP:
        present[d, d] = False
    elif diag_mode == DIAG_FILL:
        present[d, d] = True
        A[d, d] = np.float32(diag_value)
    else:
        assert diag_mode == DIAG_KEEP
    if drop_truncated_zero:
        present &= ~dropped(A)
    rows, cols = np.nonzero(present)          # row-major
    return _rowptr(rows, n), cols.astype(np.int32), A[rows, cols]


def csr_from_coo_weighted_ref(src, dst, w, n, diag_mode=DIAG_KEEP, diag_value=0.0, keep_duplicates=False, drop_truncated_zero=False):
    """Form (b), any n and either duplicate rule: (rowptr int64, colidx int32, vals float32) of gnnx_csr_from_coo_weighted.
    Given self loops leave the list unless DIAG_KEEP; DIAG_FILL appends one (i, i, diag_value) per vertex BEHIND the list; a stable
    sort by (r, c) keeps list order inside a run of equal pairs, of which the last entry wins unless duplicates are kept; then the
    drop rule per surviving entry."""
    r, c = _endpoints(src, dst, n)
    v = np.asarray(w, dtype=np.float32).reshape(-1)
    assert v.shape == r.shape and diag_mode in (DIAG_KEEP, DIAG_STRIP, DIAG_FILL)
    if diag_mode != DIAG_KEEP:
        keep = r != c
        r, c, v = r[keep], c[keep], v[keep]
    if diag_mode == DIAG_FILL:
        d = np.arange(n, dtype=np.int64)
        r, c, v = np.concatenate([r, d]), np.concatenate([c, d]), np.concatenate([v, np.full(n, diag_value, dtype=np.float32)])
    order = np.argsort(r * n + c, kind="stable")
    r, c, v = r[order], c[order], v[order]
    if not keep_duplicates and r.size:
        tail = np.concatenate([(r[1:] != r[:-1]) | (c[1:] != c[:-1]), [True]])
        r, c, v = r[tail], c[tail], v[tail]
    if drop_truncated_zero:
        keep = ~dropped(v)
        r, c, v = r[keep], c[keep], v[keep]
    return _rowptr(r, n), c.astype(np.int32), v


def degree_norm_ref(rowptr, colidx, n_rows, pow_table, s_cols=None, s_rows=None):
    """(s, norm) of gnnx_degree_norm_f32.  s = pow_table[deg + 1] (pow_table[k] = the host libm's powf(k, -0.5f)).
    norm_i = fl(fl(sum of s_cols[c_p], p from the row's last position down, every add separately rounded) * s_rows[i]).
    s_cols None: columns index s itself (a square graph); s_rows None: the rows' own s (the call that writes d_s); s_rows given:
    the call with d_s == NULL, where the caller's column-indexed vector is also row-indexed."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    assert rowptr.shape[0] == n_rows + 1
    deg = np.diff(rowptr)
    s = np.asarray(pow_table, dtype=np.float32)[deg + 1]
    cols = s if s_cols is None else np.asarray(s_cols, dtype=np.float32)
    rows = s if s_rows is None else np.asarray(s_rows, dtype=np.float32)[:n_rows]
    norm = spmm_ref(rowptr, colidx, cols[:, None], rowscale=rows)[:, 0]
    return s, norm


# ---------------------------------------------------------------------------------------------- cases of the GPU test
def rows_with_lengths(lengths, n_cols, seed):
    """A CSR with exactly these row lengths and sorted, distinct, seeded columns in [0, n_cols): (rowptr int64, colidx int32)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.min() >= 0 and lengths.max() <= n_cols
    cols = [np.sort(rng.choice(n_cols, size=int(L), replace=False)) for L in lengths]
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), np.concatenate(cols).astype(np.int32)


REQUIRED_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1057, 4097)
NORM_COLS = 5989          # 64 * 93 + 37: the square (padded) call ends in a partial block too
NORM_SEED = 4101


def norm_row_lengths():
    """The row lengths of the degree-block test, 293 rows = 4 blocks of 64 (what one wavefront of norm_long_kernel looks at) + 37:
      block 0  seven long rows: lane 0 (4097 = 64 * 64 + 1), lanes 17 / 18 and 62 / 63 adjacent, 1057 (the first degree whose libm
               powf is not the rounded rsqrt);
      block 1  no long row; 0, 1, 63, 64, 65, 127 and seeded lengths below 128;
      block 2  long rows either side of two and three chunks (191 .. 193, 255, 256);
      block 3  eight seeded long rows of 128 .. 700 entries between short ones;
      block 4  37 rows, long rows at lane 3 and at the very last row (n_rows - 1, lane 36)."""
    rng = np.random.default_rng(NORM_SEED)
    L = rng.integers(0, LONG_ROW, size=293)
    L[0], L[5], L[17], L[18], L[40], L[62], L[63] = 4097, 129, 191, 192, 1057, 257, 128
    L[64:70] = (0, 1, 63, 64, 65, 127)
    L[127] = 127
    L[128], L[130], L[131], L[160], L[191] = 193, 255, 256, 128, 129
    L[192 + rng.choice(64, size=8, replace=False)] = rng.integers(LONG_ROW, 701, size=8)
    L[259], L[292] = 320, 449
    return L


def norm_s_cols(n=NORM_COLS, seed=NORM_SEED + 1):
    """A caller's s of n entries with a spread of magnitudes, +-2^-k * u with k in 0 .. 11 and u in [0.5, 1), negative on the lower
    half of the column ids and positive on the upper half: a row's sum first grows over its upper columns and then cancels over the
    lower ones, so the rounding of the large partial sums is many units of the small result's last place, and the order of the
    additions or any regrouping of them shows in the bits of almost every row (proved by tests/test_graph_ref_cpu.py)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.5, 1.0, size=n).astype(np.float32)
    sign = np.where(np.arange(n) >= n // 2, 1.0, -1.0).astype(np.float32)
    return (sign * np.ldexp(u, -rng.integers(0, 12, size=n).astype(np.int32))).astype(np.float32)


# weights at which `(int)w != 0` and "-1 < w < 1 is dropped" could part, or at which host and device conversions differ
SPECIAL_WEIGHTS = np.array([0.0, -0.0, 1e-45, 0.99999994, -0.99999994, 1.0, -1.0, 2.0 ** 31, -2.0 ** 31, 3e38, -3e38,
                            np.inf, -np.inf, np.nan], dtype=np.float32)


def special_weight_list():
    """(src, dst, w, n): every special weight v_j three times -- alone at (3j, 3j + 1); as the LAST of a run of three at
    (3j + 1, 3j), behind 5.0 and -7.0, so a dropped v_j must take the whole pair with it; as a self loop (3j + 2, 3j + 2), behind
    an earlier 4.0.  The earlier entries of all runs come first in the list, the special values last."""
    k = len(SPECIAL_WEIGHTS)
    j = np.arange(k, dtype=np.int32)
    src = np.concatenate([3 * j + 1, 3 * j + 2, 3 * j + 1, 3 * j, 3 * j + 1, 3 * j + 2])
    dst = np.concatenate([3 * j, 3 * j + 2, 3 * j, 3 * j + 1, 3 * j, 3 * j + 2])
    w = np.concatenate([np.full(k, 5.0), np.full(k, 4.0), np.full(k, -7.0), SPECIAL_WEIGHTS, SPECIAL_WEIGHTS, SPECIAL_WEIGHTS])
    return src.astype(np.int32), dst.astype(np.int32), w.astype(np.float32), 3 * k + 1


UNWEIGHTED_FLAGS = (0, KEEP_SELF_LOOPS, KEEP_DUPLICATES, KEEP_SELF_LOOPS | KEEP_DUPLICATES)
# (diag_mode, keep_duplicates, drop_truncated_zero): the weighted builder's 3 x 2 x 2 grid
WEIGHTED_GRID = tuple((m, kd, dz) for m in (DIAG_KEEP, DIAG_STRIP, DIAG_FILL) for kd in (False, True) for dz in (False, True))

RMAT = (3001, 60000, 901)     # n, E, seed of the seeded R-MAT list


def bits(v):
    """float32 values as their uint32 bit patterns: -0.0 differs from 0.0 and a NaN equals itself."""
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
