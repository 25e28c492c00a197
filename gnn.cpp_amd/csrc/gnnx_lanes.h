// What a lane of the lane-group kernels (gnnx_heads.hip, gnnx_reduce.hip, gnnx_pool.hip) holds -- one feature or four -- and the
// element-wise steps on it, once.  Every step is one rounding per element, written so that no product is contracted into a sum; the
// units keep -ffp-contract=off and their own pragma besides.
#pragma once
#include "gnnx_common.h"

#pragma clang fp contract(off)

namespace gnnx {

template <int VEC> struct Piece;
template <> struct Piece<1> { using F = float; using I = int32_t; };
template <> struct Piece<4> { using F = float4; using I = int4; };

__device__ __forceinline__ void clear(float &a) { a = 0.f; }
__device__ __forceinline__ void clear(float4 &a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void none(int32_t &p) { p = -1; }   // "no position yet"
__device__ __forceinline__ void none(int4 &p) { p = make_int4(-1, -1, -1, -1); }
__device__ __forceinline__ float add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float mul(float x, float v) { return x * v; }
__device__ __forceinline__ float4 mul(float4 x, float v) { return make_float4(x.x * v, x.y * v, x.z * v, x.w * v); }

// the value t at position p meets the running (value, position): the first one is taken as it is (never a sentinel: a run of -inf
// keeps its first), a later one only when it is strictly better -- of equal values the first stays
__device__ __forceinline__ void meet(float &val, int32_t &pos, float t, int32_t p)
{
    const bool take = pos < 0 || t > val;
    val = take ? t : val;
    pos = take ? p : pos;
}
__device__ __forceinline__ void meet(float4 &val, int4 &pos, float4 t, int32_t p)
{
    meet(val.x, pos.x, t.x, p);
    meet(val.y, pos.y, t.y, p);
    meet(val.z, pos.z, t.z, p);
    meet(val.w, pos.w, t.w, p);
}

}  // namespace gnnx
