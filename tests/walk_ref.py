"""A restatement of the random walks (include/gnnx.h "random walks") in Python integers, Python floats and plain loops, independent of
the kernel's method: every key is masked to 64 bits by hand, a row is a Python list, membership in the previous vertex's row is `in` on
a set, the thresholds come from Python floats (the same doubles as the contract's), the fallback is a running sum.  `node2vec_probs`
enumerates the distribution the steps draw from with exact rationals, for tests/test_walk_cpu.py."""
import math
from fractions import Fraction

import numpy as np

from tests.negative_ref import GOLDEN, MASK64, fin

DOMAIN = 0x77616C6B73746570   # "walkstep"
TRIES = 64                    # GNNX_WALK_TRIES (tests/test_walk_cpu.py holds it against the header)


def h(seed, w, t, a):
    """h(w, t, a) of the contract."""
    s = fin((int(seed) & MASK64) ^ DOMAIN)
    inner = fin(s ^ ((((int(w) << 32) | int(t)) * GOLDEN) & MASK64))
    return fin(inner ^ ((int(a) * GOLDEN) & MASK64))


def thresholds(p, q):
    """(thr_a, thr_b, thr_c): candidate == previous vertex / stored in its row / otherwise."""
    ws = (1.0 / float(p), 1.0, 1.0 / float(q))
    M = max(ws)
    return tuple(min(1 << 32, int(math.floor(w / M * 4294967296.0))) for w in ws)


def classify(x, u, row_u):
    """0, 1, 2: the class of candidate x at a step that came from u, whose row is the set row_u."""
    return 0 if x == u else 1 if x in row_u else 2


def step_ref(seed, w, t, row_v, u, row_u, thr, tries=TRIES):
    """One step from a vertex with the non-empty row `row_v` (a list) that came from u (None: the uniform step), row_u a set.
    -> (next, took_fallback, zero_weight)."""
    d = len(row_v)
    if u is None:
        return row_v[(h(seed, w, t, 0) * d) >> 64], False, False
    for a in range(tries):
        x = row_v[(h(seed, w, t, 2 * a) * d) >> 64]
        if (h(seed, w, t, 2 * a + 1) >> 32) < thr[classify(x, u, row_u)]:
            return x, False, False
    weights = [thr[classify(x, u, row_u)] for x in row_v]
    W = sum(weights)
    hh = h(seed, w, t, 2 * tries)
    if W == 0:
        return row_v[(hh * d) >> 64], True, True
    r = (hh * W) >> 64
    acc = 0
    for x, wt in zip(row_v, weights):
        acc += wt
        if acc > r:
            return x, True, False
    raise AssertionError("r < W: the scan ends inside the row")


def walks_ref(rowptr, colidx, starts, L, seed, p=1.0, q=1.0, walk_base=0, general=False):
    """(walks int32 [n_walks, L + 1], n_fallback_steps, n_zero_weight_steps).  general: take the rejection path even for p == q == 1
    (the contract says its bits equal the uniform path's)."""
    rowptr = [int(v) for v in rowptr]
    colidx = [int(v) for v in colidx]
    n = len(rowptr) - 1
    uniform = float(p) == 1.0 and float(q) == 1.0 and not general
    thr = thresholds(p, q)
    row = lambda v: colidx[rowptr[v]:rowptr[v + 1]]   # noqa: E731
    walks = np.full((len(starts), L + 1), -1, dtype=np.int32)
    n_fb = n_zero = 0
    for x, start in enumerate(starts):
        w = walk_base + x
        v = int(start)
        if not 0 <= v < n:
            continue
        walks[x, 0] = v
        u = None
        for t in range(L):
            if not 0 <= v < n or not row(v):
                break
            second = not uniform and t >= 1
            nxt, fb, zero = step_ref(seed, w, t, row(v), u if second else None, set(row(u)) if second else None, thr)
            n_fb += fb
            n_zero += zero
            walks[x, t + 1] = nxt
            u, v = v, nxt
    return walks, n_fb, n_zero


def pairs_ref(walks, window):
    """(src, dst) of ops.walk_pairs: offset-major, then position, then walk; each pair followed by its reverse; pairs with a -1 dropped."""
    walks = np.asarray(walks)
    n, L = walks.shape[0], walks.shape[1] - 1
    src, dst = [], []
    for o in range(1, window + 1):
        for a in range(0, L - o + 1):
            for x in range(n):
                i, j = int(walks[x, a]), int(walks[x, a + o])
                if i < 0 or j < 0:
                    continue
                src += [i, j]
                dst += [j, i]
    return np.array(src, dtype=np.int32), np.array(dst, dtype=np.int32)


def node2vec_probs(row_v, u, row_u, p, q):
    """The node2vec transition probabilities over the entries of row_v, as Fractions of the integer thresholds (the distribution both the
    rejection and the fallback draw from, up to the 2^-64 bias of the multiply-high)."""
    thr = thresholds(p, q)
    wts = [thr[classify(x, u, set(row_u))] for x in row_v]
    return [Fraction(wt, sum(wts)) for wt in wts]
