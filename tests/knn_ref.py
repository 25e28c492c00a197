"""NumPy / Python-integer restatement of gnnx_knn_f32 (include/gnnx.h "nearest neighbours"), and the inputs of its tests.

Distances: float32 ARRAY operations in the contract's order -- one subtraction, one product, one sum per feature, each rounded once to
float32 (NumPy's element-wise loops fuse nothing); the dtype is asserted after every step.  Selection: per query the 64-bit keys
ukey(d) << 32 | c as PYTHON integers, sorted.  Nothing here looks at how the kernel maps queries to lanes."""
import numpy as np

MAX_K = 64                                    # GNNX_KNN_MAX_K
EXCLUDE_SELF, NEAREST_FIRST = 1, 2            # GNNX_KNN_EXCLUDE_SELF / GNNX_KNN_NEAREST_FIRST
REG_FEAT, TILE, TILE_LDS = 64, 64, 16         # GNNX_KNN_REG_FEAT / GNNX_KNN_TILE / GNNX_KNN_TILE_LDS
FULL_LANES = 262144                           # GNNX_KNN_FULL_LANES
GROUP_FLOATS = 128                            # GNNX_KNN_GROUP_FLOATS
REG_CELLS = (2, 3, 4, 8, 16, 32, 64)
QNAN, INF = 0x7FC00000, 0x7F800000
LOW = 0xFFFFFFFF


def distances(Q, X):
    """[m, n] float32: acc = +0; per feature t = q - c; p = t * t; acc = acc + p."""
    Q, X = np.asarray(Q), np.asarray(X)
    assert Q.dtype == np.float32 and X.dtype == np.float32 and Q.shape[1] == X.shape[1]
    acc = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for f in range(X.shape[1]):
            t = Q[:, f:f + 1] - X[None, :, f]
            assert t.dtype == np.float32
            p = t * t
            assert p.dtype == np.float32
            acc = acc + p
            assert acc.dtype == np.float32
    return acc


def distances_fma(Q, X):
    """The WRONG chain acc = fma(t, t, acc): t * t is exact in float64, the sum is rounded to float32 once."""
    Q, X = np.asarray(Q, dtype=np.float32), np.asarray(X, dtype=np.float32)
    acc = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float32)
    for f in range(X.shape[1]):
        t = (Q[:, f:f + 1] - X[None, :, f]).astype(np.float64)
        acc = (t * t + acc.astype(np.float64)).astype(np.float32)
    return acc


def distances_f64(Q, X):
    """The WRONG chain with a (double) accumulator, rounded to float32 at the end."""
    Q, X = np.asarray(Q, dtype=np.float32), np.asarray(X, dtype=np.float32)
    acc = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float64)
    for f in range(X.shape[1]):
        t = (Q[:, f:f + 1] - X[None, :, f]).astype(np.float64)
        acc = acc + t * t
    return acc.astype(np.float32)


def ukeys(d):
    """uint32 [..]: 0xFFFFFFFF for a NaN, else the bit pattern (the chain gives neither a negative value nor -0)."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    u = d.view(np.uint32).copy()
    u[np.isnan(d)] = LOW
    assert not ((u >> 31) & (u != LOW)).any()
    return u


def segments(ptr, total):
    ptr = [0, total] if ptr is None else [int(v) for v in ptr]
    assert ptr[0] == 0 and ptr[-1] == total and all(a <= b for a, b in zip(ptr, ptr[1:]))
    return ptr


def sorted_keys(X, Q=None, segptr=None, qsegptr=None, dist_fn=distances):
    """Per query the ascending list of the Python-integer keys of ALL candidates of its segment."""
    X = np.asarray(X)
    Qm = X if Q is None else np.asarray(Q)
    cp = segments(segptr, X.shape[0])
    qp = cp if Q is None else segments(qsegptr, Qm.shape[0])
    assert len(cp) == len(qp)
    out = [None] * Qm.shape[0]
    for b in range(len(cp) - 1):
        (c0, c1), (q0, q1) = cp[b:b + 2], qp[b:b + 2]
        if q0 == q1:
            continue
        u = ukeys(dist_fn(Qm[q0:q1], X[c0:c1]))
        keys = (u.astype(np.uint64) << np.uint64(32)) | np.arange(c0, c1, dtype=np.uint64)[None, :]
        for i, row in enumerate(keys.tolist()):
            assert all(type(v) is int for v in row[:1])
            out[q0 + i] = sorted(row)
    return out


def select(keys, k, flags=0):
    """(idx int32 [m, k], dist bits uint32 [m, k]) of the contract from sorted_keys' lists."""
    m = len(keys)
    idx = np.full((m, k), -1, dtype=np.int32)
    bits = np.full((m, k), INF, dtype=np.uint32)
    for i, row in enumerate(keys):
        if flags & EXCLUDE_SELF:
            row = [v for v in row if (v & LOW) != i]
        kept = row[:k]
        if not flags & NEAREST_FIRST:
            kept = sorted(kept, key=lambda v: v & LOW)
        for j, v in enumerate(kept):
            idx[i, j] = v & LOW
            bits[i, j] = QNAN if (v >> 32) == LOW else v >> 32
    return idx, bits


def knn_ref(X, k, Q=None, segptr=None, qsegptr=None, flags=0, dist_fn=distances):
    return select(sorted_keys(X, Q, segptr, qsegptr, dist_fn), k, flags)


def dispatch(n, m, n_feat, n_seg, k):
    """(form, G) by the header's rule: form = the register cell NF or "lds"; G lanes per query."""
    form = "lds" if n_feat > REG_FEAT else min(c for c in REG_CELLS if c >= n_feat)
    gm = 1
    while gm < 64 and m * gm < FULL_LANES:
        gm *= 2
    gs = 1
    while gs < 64 and gs * 2 * 2 * k <= n // n_seg:
        gs *= 2
    gw = 1
    while gw < 64 and gw * 2 * (64 if form == "lds" else form) <= GROUP_FLOATS:
        gw *= 2
    return form, min(gm, gs, gw)


ALL_CELLS = {(f, g) for f in REG_CELLS + ("lds",) for g in (1, 2, 4, 8, 16, 32, 64) if g * (64 if f == "lds" else f) <= GROUP_FLOATS}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def exact_points(seed, n, n_feat):
    """Integer coordinates in [-8, 8]: every distance is an integer far below 2^24 -- exact in any order, ties everywhere."""
    return np.random.default_rng(seed).integers(-8, 9, size=(n, n_feat)).astype(np.float32)


def rounded_points(seed, n, n_feat):
    """Uniform float32 in [-1, 1): every step of the chain rounds."""
    return (np.random.default_rng(seed).random((n, n_feat), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def case(name, sizes, n_feat, k, family="exact", qsizes=None, special=None):
    """sizes: candidates per segment; qsizes: queries per segment (None: the queries are the candidates)."""
    return dict(name=name, sizes=list(sizes), qsizes=None if qsizes is None else list(qsizes), n_feat=n_feat, k=k, family=family, special=special)


def cases():
    """The shapes of tests/test_gpu_knn.py.  Together they reach every cell of the dispatch (ALL_CELLS)."""
    out = []
    for fam in ("exact", "rounded"):
        for k in (1, 2, 7, 16, 17, 63, 64):                                   # every k, one cloud of 300 and a mixed batch
            out.append(case(f"{fam}-k{k}-one300", [300], 3, k, fam))
            out.append(case(f"{fam}-k{k}-mixed", [0, 1, 2, k, k + 1, 0, 63, 64, 65, 0], 3, k, fam))
        for F in (1, 2, 3, 4, 5, 16, 32, 63, 64, 65, 130):                    # every form; 63 / 64 / 65: the hand-over
            out.append(case(f"{fam}-F{F}-mixed", [65, 0, 17, 300, 1, 64], F, 7, fam))
            out.append(case(f"{fam}-F{F}-bip", [40, 0, 9, 130], F, 5, fam, qsizes=[3, 20, 0, 70]))
        for F in (3, 130):                                                    # segment sizes around both tile sizes
            out.append(case(f"{fam}-F{F}-tiles", [15, 16, 17, 63, 64, 65, 127, 128, 129], F, 16, fam))
    # the lane groups by segment size: k = 1, one cloud of n points gives Gs = the largest power of two <= n / 4, capped by the
    # form's Gw -- every cell of every form
    for F in (2, 3, 4, 8, 16, 32, 64, 65):
        for n in (3, 5, 9, 17, 33, 65, 129):
            out.append(case(f"groups-F{F}-n{n}", [n], F, 1, "exact" if n % 2 else "rounded"))
        out.append(case(f"groups-F{F}-k2", [257, 256], F, 2, "rounded"))
    # the lane groups by m: bipartite calls on 8 or 16 candidates (k = 1: Gs = 4 or 8) with m on the seams of Gm = 1 | 2 | 4 | 8
    for m in (FULL_LANES, FULL_LANES - 1, FULL_LANES // 2, FULL_LANES // 2 - 1, FULL_LANES // 4, FULL_LANES // 4 - 1):
        out.append(case(f"seam-m{m}", [16 if m <= FULL_LANES // 4 else 8], 2, 1, "exact", qsizes=[m]))
    out.append(case("no-candidates", [0, 0], 3, 4, qsizes=[3, 2]))           # n == 0: rows of pads
    out.append(case("no-queries", [5, 4], 3, 4, qsizes=[0, 0]))              # m == 0: nothing is written
    out.append(case("nothing", [0], 3, 4))
    out.append(case("identical", [70, 5], 3, 7, special="identical"))
    out.append(case("nonfinite", [66, 20], 4, 9, special="nonfinite"))
    out.append(case("nonfinite-lds", [40], 70, 9, special="nonfinite"))
    return out


def inputs(c, seed=0):
    """(X, Q or None, segptr, qsegptr) of a case."""
    gen = exact_points if c["family"] == "exact" else rounded_points
    n, F = sum(c["sizes"]), c["n_feat"]
    X = gen(1000 + seed, n, F)
    if c["special"] == "identical":
        X[:] = X[0]
    if c["special"] == "nonfinite":
        rng = np.random.default_rng(77)
        for val in (np.inf, -np.inf, np.nan):
            X[rng.integers(0, n, size=max(n // 8, 1)), rng.integers(0, F, size=max(n // 8, 1))] = val
    Q = None if c["qsizes"] is None else gen(2000 + seed, sum(c["qsizes"]), F)
    return X, Q, ptr_of(c["sizes"]), None if Q is None else ptr_of(c["qsizes"])
