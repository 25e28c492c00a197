"""Bars of the bf16 dense segment attention calls (include/gnnx.h "dense segment attention, bf16 operands") and the host rounding of their
operands.  The reference is tests/attn_ref.py on tests/segment_attn_ref.py's all-pairs entry list, fed the SAME bf16-rounded values.

c of each bar |got - ref| <= c * 2^-24 * S, counted from the header's ORDER as tests/segment_attn_ref.py counts the f32 calls': a sum of
length L in the matrix pipe is L roundings on one chain, but a product of two bf16 is exact in f32 and counts nothing.  Each weight
operand that is narrowed to bf16 is allowed 2^15 units of 2^-24 (2^-9 relative), added to c of the outputs it feeds and to no other:
x -> Y, alpha -> dV, ds -> dQ and dK; rowmax, rowsum and dot take none.  A single bf16 term is only good to 2^-8 (half of the spacing
2^-7 just above a power of two) and was seen to pass the dV bar (1.0024 at (8, 8)), so the kernels give the operand as hi + lo, two bf16
terms, good to 2^-16 = 2^8 units, and two adds a k-step where one term has one: both are far inside the allowance, which stays."""
import numpy as np

from tests.segment_attn_ref import tiles

BF16 = 2 ** 15


def to_bf16(a):
    """float32 values rounded to nearest even onto bf16's grid (finite input), still float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def c_s(D):           # D adds of exact products, the multiply by scale
    return D + 1


def c_dot(D):         # float(G) * Y is a rounded f32 product;  a lane adds at most D non-zero terms (the padding adds exact zeros);  the exchange
    return 1 + D + 1


def c_z(n, D):        # x: c_s + 5;  the tile's sum (16 adds, the exchange);  per tile z * r, the add, r's expf (4);  r's subtractions telescope (2)
    return c_s(D) + 5 + 17 + 6 * tiles(n) + 2


def c_Y(n, D):        # N: x and its rounding to bf16, 32 adds a tile, per tile N * r and r's expf, the telescope;  z: c_z;  the division
    return (c_s(D) + 5 + BF16 + 37 * tiles(n) + 2) + c_z(n, D) + 1


def c_ds(D):          # alpha: c_s + 5 and its division;  dP's D adds;  dot, handed over rounded;  the subtraction, the product
    return (c_s(D) + 6) + D + 1 + 2


def c_dQ(n, D):       # ds and its rounding to bf16, 32 adds a tile, the multiply by scale
    return c_ds(D) + BF16 + 32 * tiles(n) + 1


def c_dV(n, D):       # alpha and its rounding to bf16, the adds, beta
    return (c_s(D) + 6) + BF16 + 32 * tiles(n) + 1


def c_dK(n, D):       # ds and its rounding to bf16, the adds, the multiply by scale, beta
    return c_ds(D) + BF16 + 32 * tiles(n) + 2
