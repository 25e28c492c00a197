"""NumPy float64 restatement of the dot-product attention calls (include/gnnx.h "dot-product attention"): the float32 operands, every
formula in float64, no lane model.  An entry is (qi, ki, ei): the row of Q / G / m / z / dot it reads, the row of K / V, the row of E --
on the forward pattern (row i, column c) that is (i, c, eidx), on the transposed one (row c, column i) it is (colidx, row, eidx_t) -- so
one restatement serves all three calls.

Bars.  Each function returns, per output, S: the float64 sum of the absolute terms of the element, and the functions at the bottom give
c, the rounded operations on the longest chain under the header's ORDER, for |got - ref| <= c * 2^-24 * S.  A softmax weight is not a
sum of terms: x = exp(s - m) carries the absolute errors of s and m as a RELATIVE error.  With S_s = scale * sum |q| (|K| + |E|) the
absolute terms of a score (so |s| <= S_s) and c_s its operations, |dx| / x <= u (c_s S_s + c_s S_m + |s - m| + 4) <= (c_s + 5) u B with
B = 1 + S_s + S_m >= 1: every term that holds a weight carries the factor B in its S (per row B = 1 + 2 max_p S_s in the forward, where
m is computed; per entry B = 1 + S_s + |m| in the backward, where m is an operand), and c_s + 5 (+ 1 for alpha's division) in its c."""
import numpy as np

from tests.gat_fused_ref import SEG, adds, dot_chain, segsum


def heads(a, H):
    return a.reshape(a.shape[0], H, -1).sum(2)


def per_feature(a, D):
    return np.repeat(a, D, axis=1)


def segmax(v, keys, n):
    out = np.full((n,) + v.shape[1:], -np.inf)
    np.maximum.at(out, keys, v)
    return out


def entry_terms(qi, ki, ei, Q, K, V, E, H, scale):
    """per entry, float64: k', v' and their absolute terms, s [nnz, H] and S_s"""
    f = lambda a, i: a[i].astype(np.float64)  # noqa: E731
    Ee = 0.0 if E is None else f(E, ei)
    t = dict(kp=f(K, ki) + Ee, vp=f(V, ki) + Ee, absk=np.abs(f(K, ki)) + np.abs(Ee), absv=np.abs(f(V, ki)) + np.abs(Ee), q=f(Q, qi))
    t["s"] = scale * heads(t["q"] * t["kp"], H)
    t["S_s"] = abs(scale) * heads(np.abs(t["q"]) * t["absk"], H)
    return t


def forward(qi, ki, ei, n, Q, K, V, E, H, scale):
    """dict(Y [n, F], m, z [n, H], S_Y, S_m, S_z); rows without entries: Y = 0, m = -inf, z = 0"""
    D = Q.shape[1] // H
    t = entry_terms(qi, ki, ei, Q, K, V, E, H, scale)
    m = segmax(t["s"], qi, n)
    x = np.exp(t["s"] - m[qi])
    z = segsum(x, qi, n)
    alpha = per_feature(x / z[qi], D)
    S_m = np.maximum(segmax(t["S_s"], qi, n), 0)
    B = 1 + 2 * S_m
    return dict(Y=segsum(alpha * t["vp"], qi, n), m=m, z=z, S_m=S_m, S_z=B * z, S_Y=per_feature(B, D) * segsum(alpha * t["absv"], qi, n))


def backward(qi, ki, ei, nq, nk, G, Q, K, V, E, H, scale, m, z, Y=None, dot=None):
    """Both backward calls from the float32 operands THEY are handed (m, z float32; Y for the row side, which computes dot; dot for the
    column side): dot, dQ (by qi), dE (per ENTRY, [nnz, F]: the caller scatters by ei), dK, dV (by ki), each with its S."""
    D = Q.shape[1] // H
    t = entry_terms(qi, ki, ei, Q, K, V, E, H, scale)
    G64 = G.astype(np.float64)
    out = {}
    if dot is None:
        dot, S_dot = heads(G64 * Y.astype(np.float64), H), heads(np.abs(G64 * Y.astype(np.float64)), H)
        out.update(dot=dot, S_dot=S_dot)
    else:
        dot, S_dot = dot.astype(np.float64), np.abs(dot.astype(np.float64))
    g = G64[qi]
    m64 = m.astype(np.float64)[qi]
    alpha = np.exp(t["s"] - m64) / z.astype(np.float64)[qi]
    aB = alpha * (1 + t["S_s"] + np.abs(m64))
    ds = alpha * (heads(g * t["vp"], H) - dot[qi])
    S_ds = aB * (heads(np.abs(g) * t["absv"], H) + S_dot[qi])
    F = lambda a: per_feature(a, D)  # noqa: E731
    out.update(dQ=scale * segsum(F(ds) * t["kp"], qi, nq), S_dQ=abs(scale) * segsum(F(S_ds) * t["absk"], qi, nq),
               dE=F(alpha) * g + scale * F(ds) * t["q"], S_dE=F(aB) * np.abs(g) + abs(scale) * F(S_ds) * np.abs(t["q"]),
               dV=segsum(F(alpha) * g, ki, nk), S_dV=segsum(F(aB) * np.abs(g), ki, nk),
               dK=scale * segsum(F(ds) * t["q"], ki, nk), S_dK=abs(scale) * segsum(F(S_ds) * np.abs(t["q"]), ki, nk))
    return out


# ---- c of each bar, from the header's ORDER ------------------------------------------------------------------------------------------
def c_s(D):           # k' = K + E, the dot's chain (product, adds, butterfly), the multiply by scale
    return 1 + dot_chain(D) + 1


def walk(d):
    """what an entry's term goes through in the forward's online sums of a row of d entries: the adds of its segment; per block of 4 the
    rescale's multiply and the 4 of r's expf; r's subtractions, which telescope to the rise of m <= 2 S_m <= 2 B; and past one segment
    the combine's adds, its multiply and w's expf and subtraction"""
    d = np.asarray(d, dtype=np.int64)
    seg = np.minimum(d, SEG)
    return seg + 5 * -(-seg // 4) + 2 + np.where(d > SEG, -(-d // SEG) + 1 + 4 + 2, 0)


def c_z(d, D):        # x: c_s + 5 (the docstring), then the walk
    return c_s(D) + 5 + walk(d)


def c_Y(d, D):        # N: x, v' = V + E, the product, the walk;  z: c_z, carried by |Y| <= S;  the division
    return (c_s(D) + 5 + 2 + walk(d)) + c_z(d, D) + 1


def c_ds(D):          # alpha: c_s + 5 and its division;  dalpha (v' = V + E, the dot's chain) >= dot's chain;  the subtraction, the product
    return (c_s(D) + 6) + (1 + dot_chain(D)) + 2


def c_dQ(d, D):       # ds, k', the product, the adds, the multiply by scale
    return c_ds(D) + 2 + adds(d) + 1


def c_dE(D):          # the worse of alpha * G (c_s + 7) and (scale * ds) * Q (c_ds + 2), the add
    return c_ds(D) + 3


def c_dV(d, D):       # alpha, the product, the adds, beta
    return (c_s(D) + 6) + 1 + adds(d) + 1


def c_dK(d, D):       # ds, the product, the adds, the multiply by scale, beta
    return c_ds(D) + 1 + adds(d) + 2
