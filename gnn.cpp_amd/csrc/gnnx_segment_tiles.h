// The tile pieces shared by the dense segment attention units (gnnx_segment_attn.hip, gnnx_segment_cross_attn.hip): a [32][DP + 4] LDS
// tile, its copy from global memory, the MFMA operand readers, the accumulator's row map and the store of a lane's own row.  Every piece
// is written for ONE wavefront: `lane` is the lane within it, and a tile belongs to the wavefront that copies and reads it.
// gnnx_segment_attn_bf16.hip has bf16 images and readers of its own and takes the segment walk, the row map, the store and the status
// checks from here.
//
// Streamed and own tiles are [32][DP + 4] floats, DP = the head width zero-padded to 16, 32, 64 or 128 (the instantiations,
// GNNX_SEG_FOR_DP); each row is loaded from global memory with 16-byte loads where D % 4 == 0 and every pointer and pitch is 16-byte
// aligned, with scalar loads into the SAME layout otherwise.  The pitch DP + 4 makes (pitch / 4) odd: the 16-byte operand reads of 16
// consecutive rows fall on 16 different 4-bank groups.
//
// MATRIX INSTRUCTIONS (v_mfma_f32_32x32x2_f32; D[m][n] += A[m][k] B[k][n], lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31] and holds
// D[rowof(r, l >> 5)][l & 31] in register r, rowof(r, hf) = (r & 3) + 8 (r >> 2) + 4 hf).
//   score_like: the streamed tile is A, read as one float4 of row l & 31 at feature 8 c + 4 (l >> 5) per four k-steps; the own tile's
//     registers (own_regs) are B.  A lane then owns ONE own row (a column of the accumulator) and 16 of the 32 streamed rows.
//   out_like: register t of the weights IS the B operand of k-step t, which pairs streamed row rowof(t, 0) of the low half-wave with
//     rowof(t, 1) of the high one; A is the streamed tile read at [rowof(t, l >> 5)][32 i + (l & 31)].  The weights never go to LDS.
#pragma once
#include "gnnx_common.h"

namespace gnnx {
namespace seg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;      // rows of an own tile and of a streamed tile: the MFMA's M and N
constexpr int kMaxDim = 128;   // the widest instantiation

__device__ __forceinline__ int rowof(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }
__device__ __forceinline__ float rescale_of(float m, float m_new) { return m == m_new ? 1.f : expf(m - m_new); }

// rows [row0, row0 + 32) of M's columns col0 .. col0 + D - 1 -> tile [32][DP + 4]; rows at or past row_end and columns past D are zeros
template <int DP, bool VEC>
__device__ __forceinline__ void copy_in(float *tile, const float *M, int64_t ld, int64_t col0, int32_t D, int64_t row0, int64_t row_end, int lane)
{
    constexpr int LD = DP + 4;
    if constexpr (VEC) {
        constexpr int CH = DP / 4;
#pragma unroll
        for (int e0 = 0; e0 < kTile * CH; e0 += kWave) {
            const int e = e0 + lane, r = e / CH, c = e % CH;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + r < row_end && 4 * c < D) v = *reinterpret_cast<const float4 *>(M + (row0 + r) * ld + col0 + 4 * c);
            *reinterpret_cast<float4 *>(tile + r * LD + 4 * c) = v;
        }
    } else {
#pragma unroll 8
        for (int e0 = 0; e0 < kTile * DP; e0 += kWave) {
            const int e = e0 + lane, r = e / DP, c = e % DP;
            tile[r * LD + c] = (row0 + r < row_end && c < D) ? M[(row0 + r) * ld + col0 + c] : 0.f;
        }
    }
}

// the lane's B operands of the score-like products: b[4 c + i] = tile[l & 31][8 c + 4 (l >> 5) + i]
template <int DP>
__device__ __forceinline__ void own_regs(const float *tile, float (&b)[DP / 2], int lane)
{
    const float *p = tile + (lane & 31) * (DP + 4) + 4 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < DP / 8; c++) {
        const float4 v = *reinterpret_cast<const float4 *>(p + 8 * c);
        b[4 * c] = v.x, b[4 * c + 1] = v.y, b[4 * c + 2] = v.z, b[4 * c + 3] = v.w;
    }
}

// acc[rowof(r, hf)][l & 31] = sum_d tile[rowof(r, hf)][d] * own[l & 31][d]
template <int DP>
__device__ __forceinline__ f32x16 score_like(const float *tile, const float (&b)[DP / 2], int lane)
{
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    const float *p = tile + (lane & 31) * (DP + 4) + 4 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < DP / 8; c++) {
        const float4 v = *reinterpret_cast<const float4 *>(p + 8 * c);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, b[4 * c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, b[4 * c + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, b[4 * c + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, b[4 * c + 3], acc, 0, 0, 0);
    }
    return acc;
}

template <int DP> constexpr int blocks_of() { return DP >= 32 ? DP / 32 : 1; }

// out[i][rowof(r, hf)] (feature 32 i + rowof) [l & 31] += sum_t tile[rowof(t, .)][feature] * w[t] of the lane that owns [l & 31]
template <int DP>
__device__ __forceinline__ void out_like(const float *tile, const f32x16 &w, f32x16 (&out)[blocks_of<DP>()], int lane)
{
    constexpr int LD = DP + 4;
    const int col = lane & 31, hf = lane >> 5;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const float *p = tile + rowof(t, hf) * LD;
#pragma unroll
        for (int i = 0; i < blocks_of<DP>(); i++) {
            float av;
            if constexpr (DP < 32) av = col < DP ? p[col < DP ? col : 0] : 0.f;   // the MFMA's rows past the padded head width
            else av = p[32 * i + col];
            out[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, w[t], out[i], 0, 0, 0);
        }
    }
}

// acc holds [feature][own row l & 31]: the lane's 4-feature groups of its own row -> f(value, register) -> M[row][col0 + feature]
template <int DP, bool VEC, class F>
__device__ __forceinline__ void store_own(const f32x16 (&acc)[blocks_of<DP>()], float *M, int64_t ld, int64_t row, int64_t col0, int32_t D, int lane, F f)
{
    float *base = M + row * ld + col0;
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int d = 32 * i + 8 * q + 4 * (lane >> 5);
            if (d >= D) continue;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = f(acc[i][4 * q + j], d + j < D ? base + d + j : base + d);
            if constexpr (VEC) {
                *reinterpret_cast<float4 *>(base + d) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (d + j < D) base[d + j] = v[j];
            }
        }
}

// the first segment g with segptr[g + 1] > row (n_seg if there is none)
__device__ __forceinline__ int32_t first_segment(const int32_t *segptr, int32_t n_seg, int64_t row)
{
    int32_t lo = 0, hi = n_seg;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (segptr[mid + 1] <= row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// body(lo, hi, active) for every non-empty segment [lo, hi) that intersects the tile [r0, r1); active: the lane's own row is in it
template <class Body>
__device__ __forceinline__ void for_segments(const int32_t *segptr, int32_t n_seg, int32_t n_rows, int64_t r0, int64_t r1, int64_t row, Body body)
{
    for (int32_t g = first_segment(segptr, n_seg, r0); g < n_seg; g++) {
        int64_t lo = segptr[g], hi = segptr[g + 1];
        if (lo >= r1) break;
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_rows ? n_rows : hi;
        if (hi > lo) body(lo, hi, row >= lo && row < hi);
    }
}

template <int DP> struct Lds { static constexpr int kFloats = kTile * (DP + 4); };

inline bool vec4(int64_t ld, const void *p) { return ld % 4 == 0 && aligned16(p); }

// what the dense segment attention calls of either operand type check before any HIP call
inline int check_self_attn(int32_t n_seg, int32_t n_rows, int32_t H, int32_t D)
{
    GNNX_REQUIRE(n_seg >= 0 && n_rows >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(H >= 1 && D >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(n_seg > 0 || n_rows == 0, GNNX_ERR_INVALID_ARG, "rows without a segment");
    GNNX_REQUIRE(D <= kMaxDim, GNNX_ERR_UNSUPPORTED, "head_dim %d > %d", D, kMaxDim);
    GNNX_REQUIRE(H <= 65535, GNNX_ERR_UNSUPPORTED, "%d heads are too many for one launch", H);
    return GNNX_OK;
}

}  // namespace seg
}  // namespace gnnx

// ONE(what, DP) for the instantiation whose padded width holds D
#define GNNX_SEG_FOR_DP(D, ONE, what)            \
    do {                                         \
        if ((D) <= 16) ONE(what, 16);            \
        else if ((D) <= 32) ONE(what, 32);       \
        else if ((D) <= 64) ONE(what, 64);       \
        else ONE(what, 128);                     \
    } while (0)
