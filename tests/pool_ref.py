"""NumPy float32 restatement of the "graph readout" contract of include/gnnx.h (gnnx_segment_pool_f32 / gnnx_segment_pool_bwd_f32),
written from the header comment, and the inputs the CPU and GPU tests share.

pool_fwd restates the contract; its keyword switches build the DELIBERATELY WRONG variants that tests/test_pool_ref_cpu.py uses to
prove that the shared inputs tell the contract's order from its neighbours (another chunk length, a descending walk, chunks counted
from global row 0, a reciprocal multiply for the mean).  Every arithmetic step is one numpy float32 operation: one IEEE rounding.
"""
import functools

import numpy as np

T = 256   # GNNX_POOL_CHUNK
OPS = ("sum", "mean", "max")


def workspace_bytes(n_rows, n_feat, chunk=T):
    """The header's formula: tiles = n_rows / T + 1; 256 + round_up_256(4 * tiles * (4 * n_feat + 1))."""
    tiles = n_rows // chunk + 1
    return 256 + (4 * tiles * (4 * n_feat + 1) + 255) // 256 * 256


def _chunk_sum(X, b, e, descending=False):
    """ONE accumulator per feature from +0 over rows b .. e - 1 ascending (the variant: descending)."""
    acc = np.zeros(X.shape[1], dtype=np.float32)
    for r in (range(e - 1, b - 1, -1) if descending else range(b, e)):
        acc = acc + X[r]
    return acc


def segment_sum(X, s, e, chunk=T, descending=False, global_chunks=False):
    """Chunks of `chunk` rows counted from the segment's own first row s (the variant: from global row 0), ((c_0 + c_1) + c_2) + ..."""
    if e <= s:
        return np.zeros(X.shape[1], dtype=np.float32)
    if global_chunks:
        cuts = [s] + list(range((s // chunk + 1) * chunk, e, chunk)) + [e]
    else:
        cuts = list(range(s, e, chunk)) + [e]
    total = None
    for b, c in zip(cuts[:-1], cuts[1:]):
        part = _chunk_sum(X, b, c, descending)
        total = part if total is None else total + part
    return total


def pool_fwd(segptr, X, op, chunk=T, descending=False, global_chunks=False, reciprocal_mean=False):
    """(Y float32 [n_seg, F], arg int32 [n_seg, F] for "max" else None)."""
    assert op in OPS and X.dtype == np.float32
    segptr = np.asarray(segptr, dtype=np.int64)
    n_seg, F = len(segptr) - 1, X.shape[1]
    Y = np.zeros((n_seg, F), dtype=np.float32)           # an empty segment: +0
    arg = np.full((n_seg, F), -1, dtype=np.int32) if op == "max" else None
    cols = np.arange(F)
    for b in range(n_seg):
        s, e = int(segptr[b]), int(segptr[b + 1])
        if e <= s:
            continue
        if op == "max":
            # the SMALLEST row that no row of the segment beats: the first occurrence of the maximum (+0 and -0 compare equal)
            first = np.argmax(X[s:e], axis=0)
            arg[b] = s + first
            Y[b] = X[s + first, cols]                    # that row's own bits
        else:
            total = segment_sum(X, s, e, chunk, descending, global_chunks)
            if op == "mean":
                ln = np.float32(e - s)
                total = total * (np.float32(1.0) / ln) if reciprocal_mean else total / ln   # ONE division
            Y[b] = total
    return Y, arg


def pool_bwd(segptr, G, op, arg=None, dX=None, beta=0.0, n_rows=None):
    """dX_new float32 [n_rows, F]; beta == 0 never reads dX, beta == 1 is one rounded add."""
    assert op in OPS and beta in (0.0, 1.0) and G.dtype == np.float32
    segptr = np.asarray(segptr, dtype=np.int64)
    n_seg, F = len(segptr) - 1, G.shape[1]
    n_rows = int(segptr[-1]) if n_rows is None else n_rows
    t = np.zeros((n_rows, F), dtype=np.float32)
    cols = np.arange(F)
    for b in range(n_seg):
        s, e = int(segptr[b]), int(segptr[b + 1])
        if e <= s:
            continue
        if op == "sum":
            t[s:e] = G[b]
        elif op == "mean":
            t[s:e] = G[b] / np.float32(e - s)            # the same single division
        else:
            t[arg[b], cols] = G[b]                       # the row that won, +0 everywhere else
    if beta == 0.0:
        return t
    return dX.astype(np.float32) + t


# ---- the shared inputs -------------------------------------------------------------------------------------------------------------------
LONG = (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 5, 40 * T + 7)
WIDEST = 516


@functools.lru_cache(maxsize=None)
def segment_table():
    """int32 segptr of about 20 000 rows: empty segments first, last and three in a row; lengths 1, 2, 63, 64, 65; every LONG length
    with short segments on both sides (so a global tile of T rows holds the tail of one long segment, whole short ones and the head
    of the next); a run of 300 segments of 1 .. 3 rows; short filler segments of 5 .. 60 rows."""
    rng = np.random.default_rng(20240611)
    lens = [0, 1, 2, 0, 0, 0, 63, 64, 65]
    for k, ln in enumerate(LONG):
        lens += [3, 7 + k, ln, 2, 5]
    lens += [LONG[2], LONG[0]]                                    # two long segments back to back
    lens += list(rng.integers(1, 4, size=300))
    lens += list(rng.integers(5, 61, size=150))
    lens += [T, 1, 0]
    segptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=segptr[1:])
    return segptr.astype(np.int32)


def all_neg_inf_segment():
    """The segment of segment_table() that max_values() fills with -inf: the first of 64 rows."""
    segptr = segment_table().astype(np.int64)
    return int(np.nonzero(np.diff(segptr) == 64)[0][0])


@functools.lru_cache(maxsize=None)
def sum_values(F=WIDEST):
    """float32 [n_rows, F] over 25 binades with both signs: association shows in the low bits of almost every sum."""
    n = int(segment_table()[-1])
    rng = np.random.default_rng(7)
    mant = rng.uniform(1.0, 2.0, size=(n, F))
    expo = rng.integers(-12, 13, size=(n, F))
    sign = rng.choice([-1.0, 1.0], size=(n, F))
    return (sign * mant * np.exp2(expo)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def max_values(F=WIDEST):
    """float32 [n_rows, F] from {-2, -1, -0.0, +0.0, 1, 2}: ties everywhere, signed zeros among them; one segment all -inf."""
    segptr = segment_table().astype(np.int64)
    rng = np.random.default_rng(11)
    pool = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], dtype=np.float32)
    X = pool[rng.integers(0, len(pool), size=(int(segptr[-1]), F))]
    # long runs without the top values, so that zeros of both signs and -1 win somewhere too
    low = rng.random(size=(len(segptr) - 1, F)) < 0.3
    for b in np.nonzero(low.any(axis=1))[0]:
        s, e = segptr[b], segptr[b + 1]
        X[s:e][:, low[b]] = np.minimum(X[s:e][:, low[b]], pool[rng.integers(0, 4, size=(e - s, int(low[b].sum())))])
    # winners outside the first chunk: in the longest segment every fourth column starts with more than T rows of the lowest value,
    # and in the segment of 2 T + 5 rows every fourth column has it everywhere but in the short last chunk
    lens = np.diff(segptr)
    big, tail = int(np.argmax(lens)), int(np.nonzero(lens == 2 * T + 5)[0][0])
    for f in range(1, F, 4):
        X[segptr[big]:segptr[big] + T + 37 + f, f] = -2.0
    X[segptr[tail]:segptr[tail] + 2 * T, 3::4] = -2.0
    b = all_neg_inf_segment()
    X[segptr[b]:segptr[b + 1]] = -np.inf
    return np.ascontiguousarray(X)


@functools.lru_cache(maxsize=None)
def grad_values(F=WIDEST):
    """float32 [n_seg, F] upstream gradient and [n_rows, F] previous dX for beta = 1."""
    segptr = segment_table()
    rng = np.random.default_rng(13)
    G = rng.standard_normal(size=(len(segptr) - 1, F)).astype(np.float32)
    dX0 = rng.standard_normal(size=(int(segptr[-1]), F)).astype(np.float32)
    return G, dX0


@functools.lru_cache(maxsize=None)
def reference(op):
    """(Y, arg) of the contract on the shared inputs at the widest width; a narrower width is its leading columns (every feature is its
    own chain).  Computed once per process, never modified."""
    X = max_values() if op == "max" else sum_values()
    Y, arg = pool_fwd(segment_table(), X, op)
    Y.setflags(write=False)
    if arg is not None:
        arg.setflags(write=False)
    return Y, arg
