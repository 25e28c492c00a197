"""A restatement of negative sampling and link ranking (include/gnnx.h "negative sampling, ranking") in Python sets, Python integers and
plain loops, independent of the kernel's method: E is a set, the r-th non-member comes from np.setdiff1d, h and r are Python integers
(no wrap-around tricks: every step is masked to 64 bits by hand), the rank counts and the four metrics are loops over floats.
`select_by_formula` is the header's closed form (r + J(r) with the self adjustment), kept here only so that tests/test_negative_cpu.py
can hold it against the set difference."""
from fractions import Fraction

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
DOMAIN = 0x6E65676174697665
MASK64 = (1 << 64) - 1
EXCLUDE_SELF = 1


def fin(v):
    """splitmix64 of a Python integer."""
    z = (v + GOLDEN) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def key(seed, i, j, t):
    """h of the contract."""
    s = fin((int(seed) & MASK64) ^ DOMAIN)
    inner = fin(s ^ ((((int(i) << 32) | int(j)) * GOLDEN) & MASK64))
    return fin(inner ^ ((int(t) * GOLDEN) & MASK64))


def excluded_set(S, i, n_cols, flags):
    E = set(int(c) for c in S)
    if (flags & EXCLUDE_SELF) and i < n_cols:
        E.add(int(i))
    return E


def candidates(S, i, n_cols, flags):
    """[0, n_cols) \\ E, ascending."""
    E = excluded_set(S, i, n_cols, flags)
    return np.setdiff1d(np.arange(n_cols, dtype=np.int64), np.fromiter(E, dtype=np.int64, count=len(E)))


def draw(seed, i, j, t, cand):
    """The draw t of entry j of row i among the ascending candidates; -1 without one."""
    count = len(cand)
    if count == 0:
        return -1
    return int(cand[(key(seed, i, j, t) * count) >> 64])


def negatives_ref(rowptr_pos, rowptr_ex, colidx_ex, n_cols, m, seed, flags=EXCLUDE_SELF):
    """(neg [nnz_pos, m] int32, n_unfilled)."""
    rowptr_pos = np.asarray(rowptr_pos, dtype=np.int64)
    rowptr_ex = np.asarray(rowptr_ex, dtype=np.int64)
    n = len(rowptr_pos) - 1
    neg = np.empty((int(rowptr_pos[-1]), m), dtype=np.int32)
    unfilled = 0
    for i in range(n):
        if rowptr_pos[i + 1] == rowptr_pos[i]:
            continue
        cand = candidates(colidx_ex[rowptr_ex[i]:rowptr_ex[i + 1]], i, n_cols, flags)
        for p in range(rowptr_pos[i], rowptr_pos[i + 1]):
            for t in range(m):
                neg[p, t] = draw(seed, i, p - rowptr_pos[i], t, cand)
            if len(cand) == 0:
                unfilled += m
    return neg, unfilled


def select_by_formula(S, i, n_cols, flags, r):
    """The header's selection: with g(x) = c_x - x and J(r) = #{x : g(x) <= r} the r-th non-member of S is r + J(r); with the self flag,
    i < n_cols and i not in S, an answer >= i becomes (r + 1) + J(r + 1)."""
    c = np.asarray(S, dtype=np.int64)
    g = c - np.arange(len(c), dtype=np.int64)
    J = lambda v: int(np.searchsorted(g, v, side="right"))  # noqa: E731
    ans = r + J(r)
    if (flags & EXCLUDE_SELF) and i < n_cols and i not in set(c.tolist()) and ans >= i:
        ans = r + 1 + J(r + 1)
    return ans


# ---- ranking ------------------------------------------------------------------------------------------------------------------------
def rank_counts_ref(s, q, neg=None):
    """(greater, equal, valid) int32 [P]: IEEE comparisons of Python floats; a draw with neg < 0 is skipped; a NaN on either side is
    counted in none of the three."""
    s = np.asarray(s, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32).reshape(len(s), -1)
    P, m = q.shape
    greater, equal, valid = (np.zeros(P, dtype=np.int32) for _ in range(3))
    for p in range(P):
        sp = float(s[p])
        for t in range(m):
            if neg is not None and neg[p][t] < 0:
                continue
            v = float(q[p, t])
            if v > sp:
                greater[p] += 1
                valid[p] += 1
            elif v == sp:
                equal[p] += 1
                valid[p] += 1
            elif v < sp:
                valid[p] += 1
    return greater, equal, valid


def metrics_ref(s, q, neg=None, ks=(10, 50, 100)):
    """The four metrics with exact rationals (Fraction) where the contract says integers: mrr as a Fraction sum, hits@K and both AUCs as
    Fractions (None where the denominator is 0).  The global AUC is the plain double loop over all non-NaN positives and all valid
    non-NaN negatives."""
    s = np.asarray(s, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32).reshape(len(s), -1)
    greater, equal, valid = rank_counts_ref(s, q, neg)
    P = len(s)
    out = {"n_pos": P, "n_valid": int(valid.sum())}
    out["mrr"] = sum(Fraction(1, 1 + int(greater[p]) + int(equal[p])) for p in range(P)) / P if P else None
    for k in ks:
        out[f"hits@{k}"] = Fraction(sum(int(greater[p]) + int(equal[p]) < k for p in range(P)), P) if P else None
    tot = int(valid.sum())
    wins2 = sum(2 * (int(valid[p]) - int(greater[p]) - int(equal[p])) + int(equal[p]) for p in range(P))
    out["auc_grouped"] = Fraction(wins2, 2 * tot) if tot else None
    negs = [float(q[p, t]) for p in range(P) for t in range(q.shape[1]) if (neg is None or neg[p][t] >= 0) and q[p, t] == q[p, t]]
    poss = [float(v) for v in s if v == v]
    out["auc"] = Fraction(auc_wins2(poss, negs), 2 * len(poss) * len(negs)) if poss and negs else None
    return out


def auc_wins2(poss, negs, pair_limit=1_000_000):
    """Twice the wins of the positives over the negatives, a tie counting one: the double loop over all pairs, taken value by value
    (every pair of one positive value and one negative value compares alike, so the loop runs over the distinct values with their
    multiplicities; -0.0 and 0.0 are one dict key, as they are one value to an IEEE comparison)."""
    def tally(values):
        c = {}
        for v in values:
            c[v] = c.get(v, 0) + 1
        return c

    cp, cn = tally(poss), tally(negs)
    if len(cp) * len(cn) <= pair_limit:
        return sum(na * nb * (2 if a > b else 1 if a == b else 0) for a, na in cp.items() for b, nb in cn.items())
    wins2, below, it = 0, 0, iter(sorted(cn.items()))      # many distinct values: one merge pass over both sorted value lists
    nxt = next(it, None)
    for a, na in sorted(cp.items()):
        while nxt is not None and nxt[0] < a:
            below += nxt[1]
            nxt = next(it, None)
        wins2 += na * (2 * below + (nxt[1] if nxt is not None and nxt[0] == a else 0))
    return wins2
