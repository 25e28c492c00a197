"""float64 restatement of the cross segment attention calls (include/gnnx.h "cross segment attention") as plain loops over segments and
heads, from the float32 operands, with S, the sum of the absolute terms of every output, as tests/attn_ref.py defines it (a term that
holds a softmax weight carries the factor B = 1 + S_s + S_m: expf turns the score's absolute error into a relative one).

c of each bar |got - ref| <= c * 2^-24 * S: the counts of tests/segment_attn_ref.py with n the streamed segment's length, plus the merge
of the four wavefronts' states.  Per wavefront the merge costs one expf (4, as r's expf is counted there), one product and one add: 6,
24 for the four; r_w's subtraction m_w - m* is on the telescoping chain already counted.  z takes the merge once (+ 24); Y takes it for N
and, through the division, for z (+ 48); dQ's merge is three adds (+ 3).  The maximum is exact, the column side has no merge."""
import numpy as np

from tests import segment_attn_ref as sr

MERGE = 24


def c_z(n, D):
    return sr.c_z(n, D) + MERGE


def c_Y(n, D):
    return sr.c_Y(n, D) + 2 * MERGE


def c_dQ(n, D):
    return sr.c_dQ(n, D) + 3


def lengths(segptr, qsegptr, n_q, n_rows):
    """(keys of every query's segment [n_q], the streamed length of every key [n_rows]); 0 for a row that no segment holds.  The column
    side streams the QUERIES of a key's segment, so its chain has their number; where the key segment is the shorter of the two its
    length is taken, which is never the wider bar."""
    nk, nq = np.zeros(n_q, np.int64), np.zeros(n_rows, np.int64)
    for g in range(len(segptr) - 1):
        nk[qsegptr[g]:qsegptr[g + 1]] = segptr[g + 1] - segptr[g]
        nq[segptr[g]:segptr[g + 1]] = min(qsegptr[g + 1] - qsegptr[g], segptr[g + 1] - segptr[g])
    return nk, nq


def forward(segptr, qsegptr, Q, K, V, H, scale):
    """dict(Y [n_q, F], m, z [n_q, H], S_Y, S_m, S_z); a query without keys: Y = 0, m = -inf, z = 0"""
    (n_q, F), D = Q.shape, Q.shape[1] // H
    Q, K, V = (a.astype(np.float64) for a in (Q, K, V))
    o = dict(Y=np.zeros((n_q, F)), S_Y=np.zeros((n_q, F)), m=np.full((n_q, H), -np.inf), z=np.zeros((n_q, H)), S_m=np.zeros((n_q, H)),
             S_z=np.zeros((n_q, H)))
    for g in range(len(segptr) - 1):
        qs, ks = slice(qsegptr[g], qsegptr[g + 1]), slice(segptr[g], segptr[g + 1])
        if qs.stop == qs.start or ks.stop == ks.start:
            continue
        for h in range(H):
            c = slice(h * D, (h + 1) * D)
            s, S_s = scale * Q[qs, c] @ K[ks, c].T, abs(scale) * np.abs(Q[qs, c]) @ np.abs(K[ks, c]).T
            m = s.max(1)
            x = np.exp(s - m[:, None])
            z, S_m = x.sum(1), S_s.max(1)
            B = 1 + 2 * S_m
            o["m"][qs, h], o["z"][qs, h], o["S_m"][qs, h], o["S_z"][qs, h] = m, z, S_m, B * z
            o["Y"][qs, c], o["S_Y"][qs, c] = (x / z[:, None]) @ V[ks, c], B[:, None] * ((x / z[:, None]) @ np.abs(V[ks, c]))
    return o


def backward(segptr, qsegptr, G, Q, K, V, Y, m, z, H, scale):
    """dot, dQ (query side), dK, dV (key side) and their S, from the float32 m, z and Y that the device calls are handed"""
    (n_q, F), n_rows, D = Q.shape, K.shape[0], Q.shape[1] // H
    G, Q, K, V, Y, m, z = (a.astype(np.float64) for a in (G, Q, K, V, Y, m, z))
    o = {k: np.zeros((n_q, F)) for k in ("dQ", "S_dQ")}
    o.update({k: np.zeros((n_rows, F)) for k in ("dK", "S_dK", "dV", "S_dV")})
    o["dot"], o["S_dot"] = (G * Y).reshape(n_q, H, D).sum(2), np.abs(G * Y).reshape(n_q, H, D).sum(2)
    for g in range(len(segptr) - 1):
        qs, ks = slice(qsegptr[g], qsegptr[g + 1]), slice(segptr[g], segptr[g + 1])
        if qs.stop == qs.start or ks.stop == ks.start:
            continue
        for h in range(H):
            c = slice(h * D, (h + 1) * D)
            q, k, v, gr = Q[qs, c], K[ks, c], V[ks, c], G[qs, c]
            s, S_s = scale * q @ k.T, abs(scale) * np.abs(q) @ np.abs(k).T
            alpha = np.exp(s - m[qs, h, None]) / z[qs, h, None]
            aB = alpha * (1 + S_s + np.abs(m[qs, h, None]))
            ds, S_ds = alpha * (gr @ v.T - o["dot"][qs, h, None]), aB * (np.abs(gr) @ np.abs(v).T + o["S_dot"][qs, h, None])
            o["dQ"][qs, c], o["S_dQ"][qs, c] = scale * ds @ k, abs(scale) * S_ds @ np.abs(k)
            o["dV"][ks, c], o["S_dV"][ks, c] = alpha.T @ gr, aB.T @ np.abs(gr)
            o["dK"][ks, c], o["S_dK"][ks, c] = scale * ds.T @ q, abs(scale) * S_ds.T @ np.abs(q)
    return o
