"""NumPy restatements of the loss, argmax and label-mask calls of include/gnnx.h (gnnx_softmax_ce*_f32, gnnx_bce_logits_f32,
gnnx_mask_to_rows, gnnx_csr_restrict, gnnx_argmax_rows_f32 / gnnx_accuracy_rows_f32), written from the header comment as plain loops,
and the inputs that tests/test_loss_ref_cpu.py, tests/test_gpu_loss.py and tests/test_gpu_mask_calls.py share.

Two kinds of input:
  * DYADIC families, on which no kernel path ever rounds.  Logits are 0.0 or a "dead" value (-inf or -200.0: expf gives exactly 1 and
    exactly 0), a row holds k in {0, 1, 2, 4, 8} zeros and n_total = 2^b.  The row sum is the integer k in any order, k + 1e-20 = k
    in f32, 1 / k is a power of two, and every gradient entry is (8 / k * [x == 0] - 8 * onehot) * 2^-(3 + b): an integer in
    [-8, 8] times a power of two.  A column sum over n <= 2^17 rows is an integer below 2^20 in those units: exact in f32 in ANY
    summation order.  The expected values come from int64 arithmetic (`dyadic_ce_int`), so the bar is bit equality.
  * general data, held per element against float64 (`softmax_ce_ref64`) with the bounds of tests/test_gpu_loss.py.
"""
import numpy as np

from tests.sddmm_ref import bce_logits_ref64 as bce_ref64  # noqa: F401  (re-exported: one restatement of the BCE formula)

DEAD_VALUES = (-np.inf, -200.0)


# ------------------------------------------------------------------ softmax cross-entropy, float64
def softmax_ce_ref64(X, target, rows=None, n_total=None):
    """(loss, dlogits, colsum, row_losses) in float64, the header's formula term by term:
        l_i = -log( exp(x_i[t_i]) / (sum_c exp(x_ic) + 1e-20) ),   loss = sum_{i listed} l_i / n_total     (no max-subtraction)
        dlogits[i, :] = (exp(x_i) / (sum_c exp(x_ic) + 1e-20) - onehot(t_i)) / n_total                      for listed rows
    dlogits is a list with one float64 row per matrix row, None where the row is not listed (the call leaves it untouched);
    colsum = the sum of the listed gradient rows; row_losses[k] belongs to the k-th listed row."""
    X = np.asarray(X, dtype=np.float64)
    n, C = X.shape
    listed = list(range(n)) if rows is None else [int(r) for r in rows]
    n_total = len(listed) if n_total is None else int(n_total)
    dlogits = [None] * n
    colsum = np.zeros(C, dtype=np.float64)
    row_losses = np.zeros(len(listed), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k, r in enumerate(listed):
            t = int(target[r])
            assert 0 <= t < C and 0 <= r < n
            e = np.exp(X[r])
            denom = 0.0
            for c in range(C):
                denom += e[c]
            denom += 1e-20
            row_losses[k] = -np.log(e[t] / denom)
            g = e / denom
            g[t] -= 1.0
            g /= n_total
            dlogits[r] = g
            colsum += g
        loss = 0.0
        for v in row_losses:
            loss += v
        loss /= n_total
    return float(loss), dlogits, colsum, row_losses


def softmax_probs64(X, rows=None):
    """float64 [n_listed, C]: exp(x) / (sum exp(x) + 1e-20) of the listed rows (the `p` of the error bounds)."""
    X = np.asarray(X, dtype=np.float64)
    if rows is not None:
        X = X[np.asarray(rows, dtype=np.int64)]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(X)
        return e / (e.sum(1, keepdims=True) + 1e-20)


# ------------------------------------------------------------------ dyadic families
def _ks(C, most):
    return [k for k in (1, 2, 4, 8) if k <= most]


def dense(seed, n, C, dead):
    """(X f32 [n, C], target i32 [n]): row i holds k_i in {1, 2, 4, 8} (k_i <= C) zeros at seeded columns, the rest `dead`; the target
    is one of the zeros.  The first and the last row have k >= 2 when C allows it, so their gradient rows are not all zero."""
    rng = np.random.default_rng(seed)
    ks = np.array(_ks(C, C))
    k = ks[rng.integers(0, len(ks), n)]
    if C >= 2:
        k[0] = k[-1] = 2
    rank = rng.random((n, C)).argsort(1).argsort(1)          # rank[i, c]: a seeded permutation of 0..C-1 per row
    X = np.where(rank < k[:, None], np.float32(0.0), np.float32(dead)).astype(np.float32)
    return X, np.argmin(rank, 1).astype(np.int32)


def edge_columns(C):
    """The columns next to every float4 boundary of the first and last lane and to both ends of a 256-class granule's row."""
    return sorted({c for c in (0, 3, 4, C - 5, C - 4, C - 1) if 0 <= c < C})


def edges(n, C, dead):
    """(X, target): the zeros of row i are k_i in {2, 4, 1} (k_i <= the number of edge columns) consecutive members of edge_columns(C),
    starting at member i, the target on the first of them -- over the rows every edge column carries mass, with and without the
    one-hot."""
    cols = edge_columns(C)
    m = len(cols)
    ks = [k for k in (2, 4, 1) if k <= m]
    X = np.full((n, C), dead, dtype=np.float32)
    t = np.zeros(n, dtype=np.int32)
    for i in range(n):
        k = ks[i % len(ks)]
        for j in range(k):
            X[i, cols[(i + j) % m]] = 0.0
        t[i] = cols[i % m]
    if ks[-1] == 1 and ks[(n - 1) % len(ks)] == 1 and m >= 2:       # the last row's gradient is not all zero: a dropped row shows in the sums
        X[n - 1, cols[n % m]] = 0.0
    return X, t


def target_dead(seed, n, C, dead):
    """(X, target): the target's logit is dead; k_i in {0, 1, 2, 4, 8} (k_i <= C - 1) zeros elsewhere.  Row i with i % 5 == 0 is
    FULLY dead (k = 0: sum = 0, denominator 1e-20): its gradient is -onehot / n_total, its row loss +inf -- as every row's here."""
    rng = np.random.default_rng(seed)
    ks = np.array([0] + _ks(C, C - 1))
    k = ks[rng.integers(0, len(ks), n)]
    k[::5] = 0
    rank = rng.random((n, C)).argsort(1).argsort(1)
    X = np.where(rank < k[:, None], np.float32(0.0), np.float32(dead)).astype(np.float32)
    return X, np.argmax(rank, 1).astype(np.int32)            # rank C - 1 >= k: never a zero


def log2_exact(n_total):
    b = int(n_total).bit_length() - 1
    assert n_total == 1 << b, "the dyadic families need n_total = 2^b"
    return b


def dyadic_ce_int(X, target, rows=None):
    """int64 (G [n_listed, C], colsum [C]) in units of 2^-(3 + b), n_total = 2^b: G = 8 / k * [x == 0] - 8 * onehot(t), k = zeros of
    the row.  Integer arithmetic only."""
    X = np.asarray(X)
    sel = np.arange(X.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    Z = (X[sel] == 0.0)
    assert np.all(Z | (X[sel] <= -200.0)), "not a dyadic input"
    k = Z.sum(1).astype(np.int64)
    assert np.all(np.isin(k, (0, 1, 2, 4, 8)))
    G = Z.astype(np.int64) * (8 // np.maximum(k, 1))[:, None]
    G[np.arange(len(sel)), np.asarray(target)[sel]] -= 8
    return G, G.sum(0)


def dyadic_to_f32(ints, n_total):
    """The float32 values of integers in units of 2^-(3 + b); the conversion is exact (checked)."""
    v = np.asarray(ints, dtype=np.float64) * 2.0 ** -(3 + log2_exact(n_total))
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v), "not representable in f32"
    return out


def softmax_ce_f32(X, target, n_total, class_order=None, row_order=None):
    """(dlogits f32 [n, C], colsum f32 [C]) by float32 NumPy operations in the kernels' operation order -- e = exp(x); sum over the
    classes in `class_order` (default ascending), one rounding per addition; + 1e-20; 1 / denominator; (e * rden - onehot) * (1 / n_total);
    column sums over the rows in `row_order`.  Used on the CPU to show that a dyadic family gives the same bits in every order."""
    X = np.asarray(X, dtype=np.float32)
    n, C = X.shape
    class_order = range(C) if class_order is None else class_order
    row_order = range(n) if row_order is None else row_order
    with np.errstate(under="ignore"):
        e = np.exp(X)
    assert e.dtype == np.float32
    s = np.zeros(n, dtype=np.float32)
    for c in class_order:
        s = s + e[:, c]
    rden = np.float32(1.0) / (s + np.float32(1e-20))
    onehot = np.zeros((n, C), dtype=np.float32)
    onehot[np.arange(n), target] = 1.0
    d = (e * rden[:, None] - onehot) * (np.float32(1.0) / np.float32(n_total))
    assert d.dtype == np.float32
    cs = np.zeros(C, dtype=np.float32)
    for r in row_order:
        cs = cs + d[r]
    return d, cs


def heavy_row_case(n, C, r, dead):
    """(X, target): every row has one zero, on its target (row loss exactly 0), but row r: x_t = -64, one other logit 0, the rest dead
    -- its loss is -log(exp(-64) / (1 + exp(-64) + 1e-20)), about 64.  The mean equals l_r / n_total iff row r is counted exactly
    once and no other row contributes."""
    assert C >= 2 and 0 <= r < n
    X = np.full((n, C), dead, dtype=np.float32)
    t = (np.arange(n) % C).astype(np.int32)
    X[np.arange(n), t] = 0.0
    X[r, t[r]] = -64.0
    X[r, (t[r] + 1) % C] = 0.0
    return X, t


# ------------------------------------------------------------------ binary cross-entropy, dyadic
def bce_dyadic(seed, n, with_zero=False):
    """(x, y) f32 [n]: x in {+-128, +-256} (exp(-|x|) = 0 in f32, log1p(0) = 0), y in {0, 1, 0.25}: every loss term max(x, 0) - x y is
    a multiple of 32 up to 256, so a sum over n <= 2^17 terms is exact in f32 in any order; every gradient is one of
    {1, 0, 0.75, -1, -0.25} / n_total.  with_zero adds x = 0 (gradient (0.5 - y) / n_total exact; loss term ln 2 is not: gradients only)."""
    rng = np.random.default_rng(seed)
    xs = np.array([128, -128, 256, -256] + ([0] if with_zero else []), dtype=np.float32)
    ys = np.array([0, 1, 0.25], dtype=np.float32)
    x, y = xs[rng.integers(0, len(xs), n)], ys[rng.integers(0, len(ys), n)]
    x[0], y[0] = 128.0, 0.25                                   # a non-zero first and last term: a dropped end is visible
    if n > 1:
        x[-1], y[-1] = -256.0, 1.0
    return x, y


def bce_dyadic_int(x, y):
    """(sum of the loss terms as an int, exact float64 sigmoid(x) - y) for a bce_dyadic input (x = 0 contributes no loss term here)."""
    x4, y4 = np.asarray(x).astype(np.int64), np.round(np.asarray(y, dtype=np.float64) * 4).astype(np.int64)
    terms4 = 4 * np.maximum(x4, 0) - x4 * y4                  # 4 * (max(x, 0) - x y)
    assert np.all(terms4 % 128 == 0)
    sig = np.where(np.asarray(x) > 0, 1.0, np.where(np.asarray(x) < 0, 0.0, 0.5))
    return int(terms4.sum()) // 4, sig - np.asarray(y, dtype=np.float64)


# ------------------------------------------------------------------ label masks
def mask_rows_ref(mask):
    """int32: the positions of the non-zero bytes, ascending."""
    out = []
    for i, b in enumerate(np.asarray(mask).astype(np.uint8).tolist()):
        if b != 0:
            out.append(i)
    return np.array(out, dtype=np.int32)


def restrict_ref(rowptr, colidx, vals, row_keep, col_keep):
    """(rowptr', colidx', vals' or None): entry (r, c) stays iff row_keep[r] != 0 (when given) and col_keep[c] != 0 (when given); the
    survivors of a row keep their stored order; the number of rows is unchanged."""
    n = len(rowptr) - 1
    rp, ci, vv = [0], [], []
    for r in range(n):
        for p in range(int(rowptr[r]), int(rowptr[r + 1])):
            c = int(colidx[p])
            if row_keep is not None and row_keep[r] == 0:
                continue
            if col_keep is not None and col_keep[c] == 0:
                continue
            ci.append(c)
            if vals is not None:
                vv.append(vals[p])
        rp.append(len(ci))
    return (np.array(rp, dtype=np.int32), np.array(ci, dtype=np.int32),
            None if vals is None else np.array(vv, dtype=np.float32))


def argmax_first_ref(X):
    """int32 [n]: the FIRST index of the maximum of each row, by a loop with `>` (-0.0 == +0.0, the infinities ordered).  NaN is
    refused: the header leaves it unspecified."""
    X = np.asarray(X, dtype=np.float32)
    if np.isnan(X).any():
        raise ValueError("argmax_first_ref: NaN (unspecified by the header)")
    out = np.zeros(X.shape[0], dtype=np.int32)
    for i, row in enumerate(X.tolist()):
        best, bi = row[0], 0
        for c in range(1, len(row)):
            if row[c] > best:
                best, bi = row[c], c
        out[i] = bi
    return out


def argmax_case(seed, n, C):
    """f32 [n, C] of values from {-2, -1, -0.0, +0.0, 1}: most rows tie, also -0.0 with +0.0.  Row r with (r + seed) % 5 = 1 is all
    -inf, = 2 holds a single +inf, = 3 has its maximum first (and only) at C - 1, = 4 is -2 but for a -0.0 / +0.0 tie (C >= 2: the
    -0.0 comes first and wins)."""
    rng = np.random.default_rng(seed)
    X = np.array([-2.0, -1.0, -0.0, 0.0, 1.0], dtype=np.float32)[rng.integers(0, 5, (n, C))]
    for r in range(n):
        kind = (r + seed) % 5
        if kind == 1:
            X[r] = -np.inf
        elif kind == 2:
            X[r, int(rng.integers(0, C))] = np.inf
        elif kind == 3:
            X[r] = -2.0
            X[r, C - 1] = 1.0
        elif kind == 4 and C >= 2:
            a = int(rng.integers(0, C - 1))
            X[r] = -2.0
            X[r, a] = -0.0
            X[r, int(rng.integers(a + 1, C))] = 0.0
    return X


# ------------------------------------------------------------------ tiny CSR patterns for the restriction
def _csr(lengths, n_cols, col_of=None):
    """(n_rows, n_cols, rowptr, colidx): row r has lengths[r] entries; entry j of row r has column col_of(r, j) (default: (3 r + 7 j) %
    n_cols, ascending in j only by accident -- the call never needs sorted rows)."""
    col_of = col_of or (lambda r, j: (3 * r + 7 * j) % n_cols)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    colidx = np.array([col_of(r, j) for r, L in enumerate(lengths) for j in range(L)], dtype=np.int32)
    return len(lengths), n_cols, rowptr, colidx


def tiny_csr_patterns():
    """name -> (n_rows, n_cols, rowptr, colidx), each named for the edge it sits on (chunks of 64 entries, the rowptr[r] >= nnz
    branch of leading / trailing empty rows)."""
    P = {}
    P["empty"] = _csr([0, 0, 0], 3)
    P["one_entry"] = _csr([0, 1, 0], 3)
    P["lead_trail_empty"] = _csr([0, 0, 3, 5, 1, 0, 0], 7)
    for L in (64, 65, 128):
        P[f"row{L}"] = _csr([0, L, 0], 131)
    P["straddle"] = _csr([40] * 9, 50)
    P["many_empty"] = _csr([1 if r % 7 == 3 else 0 for r in range(200)], 200)
    P["rect"] = _csr([2, 0, 70, 1, 9], 300)
    P["unsorted_dups"] = _csr([5, 70, 0, 6], 12, col_of=lambda r, j: (11 - (j // 2)) % 12)      # descending, each column twice
    P["one_row"] = _csr([130], 40)
    return P


def tiny_vals(nnz):
    return (np.arange(nnz, dtype=np.float32) * np.float32(0.5) - np.float32(3.0)).astype(np.float32)
