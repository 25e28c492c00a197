// The dot product of the edge-score kernels (gnnx_sddmm.hip, gnnx_heads.hip), once.  Its ORDER is part of the contract of
// include/gnnx.h ("edge scores", "multi-head attention") and a function of the row length F alone: Q = ceil(F / 4) chunks of four
// features, a lane group of G = min(64, pow2 >= Q) lanes, lane l owns chunks l, l + G, ... and adds their products in ascending f
// to ONE accumulator, each product rounded before the sum; the G accumulators meet in an xor butterfly (s = 1, 2, .., G / 2).
// "Head h carries the bits of the single-head call on slab h" holds because both units take every step of that order from here.
// The GATv2 score (gnnx_gatv2.hip) sums in the same order; only its chunk step differs (add_leaky_chunk).
#pragma once
#include "gnnx_common.h"

#pragma clang fp contract(off)

namespace gnnx {

constexpr int kEntriesPerGroup = 32;   // consecutive entries of one lane group (a multiple of kInFlight)
constexpr int kInFlight = 4;           // R rows requested before the first is consumed

// the smallest row r with rowptr[r + 1] > p (p < rowptr[n_rows]): the row that stores entry p, empty rows skipped
__device__ __forceinline__ int32_t row_of_entry(const int32_t *rowptr, int32_t n_rows, int64_t p)
{
    int32_t lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)rowptr[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// features 4 q .. 4 q + 3 of a row of F features (zero behind the row's end; the consumer never adds those)
template <bool VEC>
__device__ __forceinline__ float4 load_chunk(const float *row, int32_t q, int32_t F)
{
    if constexpr (VEC) {
        return *reinterpret_cast<const float4 *>(row + 4 * (int64_t)q);
    } else {
        const int32_t f = 4 * q;
        float4 v;
        v.x = row[f];                      // q < Q: the chunk's first feature exists
        v.y = f + 1 < F ? row[f + 1] : 0.f;
        v.z = f + 2 < F ? row[f + 2] : 0.f;
        v.w = f + 3 < F ? row[f + 3] : 0.f;
        return v;
    }
}

// acc = acc + (l * r) over the chunk's features in ascending f: the product is rounded, then the sum
template <bool VEC>
__device__ __forceinline__ float add_chunk(float acc, const float4 &l, const float4 &r, int32_t q, int32_t F)
{
    const int32_t f = 4 * q;
    acc = acc + (l.x * r.x);
    if (VEC || f + 1 < F) acc = acc + (l.y * r.y);
    if (VEC || f + 2 < F) acc = acc + (l.z * r.z);
    if (VEC || f + 3 < F) acc = acc + (l.w * r.w);
    return acc;
}

// the GATv2 score's chunk step (gnnx_gatv2.hip): acc = acc + (a * leaky(l + r)) in the same feature order -- the sum u = l + r, the
// slope product u * slope (u <= 0, a zero included) and the term a * e are each rounded before the add
__device__ __forceinline__ float leaky(float u, float slope) { return u > 0.f ? u : u * slope; }
__device__ __forceinline__ float4 leaky(float4 u, float slope)
{
    return make_float4(leaky(u.x, slope), leaky(u.y, slope), leaky(u.z, slope), leaky(u.w, slope));
}
__device__ __forceinline__ float leaky_term(float l, float r, float a, float slope) { return a * leaky(l + r, slope); }

template <bool VEC>
__device__ __forceinline__ float add_leaky_chunk(float acc, const float4 &l, const float4 &r, const float4 &a, float slope, int32_t q,
                                                 int32_t F)
{
    const int32_t f = 4 * q;
    acc = acc + leaky_term(l.x, r.x, a.x, slope);
    if (VEC || f + 1 < F) acc = acc + leaky_term(l.y, r.y, a.y, slope);
    if (VEC || f + 2 < F) acc = acc + leaky_term(l.z, r.z, a.z, slope);
    if (VEC || f + 3 < F) acc = acc + leaky_term(l.w, r.w, a.w, slope);
    return acc;
}

template <int G>
__device__ __forceinline__ float butterfly(float acc)
{
#pragma unroll
    for (int s = 1; s < G; s <<= 1) acc = acc + __shfl_xor(acc, s, 64);   // partners stay inside the aligned group of G lanes
    return acc;
}

}  // namespace gnnx
