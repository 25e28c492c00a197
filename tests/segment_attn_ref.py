"""Reference and bars of the dense segment attention calls (include/gnnx.h "dense segment attention"): segptr is expanded into the
all-pairs entry list of each segment and handed to tests/attn_ref.py (float64 from the float32 operands on, E = None), which returns S,
the sum of the absolute terms, for every output.

c of each bar |got - ref| <= c * 2^-24 * S, from the header's ORDER.  The matrix pipe's internal order is not documented, so a dot or a
sum of length L counts as L roundings on ONE chain (the most any order puts on one term), plus one for the product.  A segment of n rows
is T = ceil(n / 32) streamed tiles; an accumulator that lives across them takes up to 32 adds per tile.  Terms that hold a softmax
weight keep attn_ref's factor 1 + S_s + S_m in S and c_s + 5 in c (expf turns the score's absolute error into a relative one)."""
import numpy as np

TILE = 32


def pairs(segptr):
    """(qi, ki, lengths per row): every (query, key) pair of every segment, query-major"""
    qi, ki = [], []
    for lo, hi in zip(segptr[:-1], segptr[1:]):
        r = np.arange(lo, hi, dtype=np.int64)
        qi.append(np.repeat(r, hi - lo)), ki.append(np.tile(r, hi - lo))
    return np.concatenate(qi), np.concatenate(ki), np.repeat(np.diff(segptr), np.diff(segptr))


def tiles(n):
    return -(-np.asarray(n, dtype=np.int64) // TILE)


def c_s(D):           # the product and D adds, the multiply by scale
    return D + 2


def c_dot(D):         # the lane's products and adds, the exchange
    return D + 1


def c_z(n, D):        # x: c_s + 5;  the tile's sum (16 adds, the exchange);  per tile z * r, the add, r's expf (4);  r's subtractions telescope (2)
    return c_s(D) + 5 + 17 + 6 * tiles(n) + 2


def c_Y(n, D):        # N: x, the product, 32 adds a tile, per tile N * r and r's expf, the telescope;  z: c_z, carried by |Y| <= S;  the division
    return (c_s(D) + 5 + 1 + 37 * tiles(n) + 2) + c_z(n, D) + 1


def c_ds(D):          # alpha: c_s + 5 and its division;  dP's chain;  dot, handed over rounded;  the subtraction, the product
    return (c_s(D) + 6) + (D + 1) + 1 + 2


def c_dQ(n, D):       # ds, the product, 32 adds a tile, the multiply by scale
    return c_ds(D) + 1 + 32 * tiles(n) + 1


def c_dV(n, D):       # alpha, the product, the adds, beta
    return (c_s(D) + 6) + 1 + 32 * tiles(n) + 1


def c_dK(n, D):       # ds, the product, the adds, the multiply by scale, beta
    return c_ds(D) + 1 + 32 * tiles(n) + 2
