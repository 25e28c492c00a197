// Dense self-attention inside the segments of a batch (graph transformers' GLOBAL attention: every vertex of a graph attends to every
// vertex of the same graph) -- include/gnnx.h "dense segment attention".  Row i of segment g = [segptr[g], segptr[g+1]), head h of width D:
//   s_ij = scale * <Q_i, K_j>_h for j in g;  m_i = max_j s_ij;  x_ij = expf(s_ij - m_i);  z_i = sum_j x_ij
//   forward    Y_i = (sum_j x_ij V_j) / z_i,  rowmax = m,  rowsum = z
//   bwd, rows  dot[i, h] = <G_i, Y_i>_h;  dQ_i = scale * sum_j ds_ij K_j
//   bwd, cols  dV_j (+)= sum_i alpha_ij G_i;  dK_j (+)= scale * sum_i ds_ij Q_i
// with alpha_ij = x_ij / z_i and ds_ij = alpha_ij (<G_i, V_j>_h - dot[i, h]).  No index array, no workspace, no atomics.
//
// WORK SPLIT.  grid = (tiles of 32 consecutive rows of the WHOLE batch) x heads, ONE wavefront per workgroup: nothing waits on another
// wavefront, and a workgroup's barriers are its own 64 lanes'.  The wavefront finds the first segment that holds a row of its tile by
// binary search in segptr and walks the segments that intersect the tile; per segment it streams that segment's rows in tiles of 32
// (starting at the segment's first row) through LDS.  The forward and the row side own 32 QUERIES and stream keys; the column side owns
// 32 KEYS and streams queries.  A row of the own tile outside the current segment and a streamed row past the segment's end are
// masked (score -inf, weight exactly 0) and never loaded: the tile's LDS rows are zero-filled.  Each output element has one
// accumulator in one lane: the same bits every run.
//
// DATA MOVEMENT.  The own tile (Q; Q and G; K and V) is copied to LDS once, read into registers as the MFMA's B operand and stays there.
// Streamed tiles are [32][DP + 4] floats in LDS, DP = the head width zero-padded to 16, 32, 64 or 128 (the instantiations); each row
// is loaded from global memory once per workgroup, with 16-byte loads where D % 4 == 0 and every pointer and pitch is 16-byte aligned,
// with scalar loads into the SAME layout otherwise.  The pitch DP + 4 makes (pitch / 4) odd: the 16-byte operand reads of 16
// consecutive rows fall on 16 different 4-bank groups.
//
// MATRIX INSTRUCTIONS (v_mfma_f32_32x32x2_f32; D[m][n] += A[m][k] B[k][n], lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31] and holds
// D[rowof(r, l >> 5)][l & 31] in register r, rowof(r, hf) = (r & 3) + 8 (r >> 2) + 4 hf).
//   score-like products  S^T = K Q^T, dP^T = V G^T (column side: S = Q K^T, dP = G V^T): the streamed tile is A, read as one float4 of row
//     l & 31 at feature 8 c + 4 (l >> 5) per four k-steps; the own tile's registers are B.  A lane then owns ONE own row (a column of
//     the accumulator) and 16 of the 32 streamed rows: maximum and sum are 15 in-register operations and one exchange with lane ^ 32.
//   output-like products  O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += G^T alpha, dK^T += Q^T dS: register t of the weights IS the B operand
//     of k-step t, which pairs streamed row rowof(t, 0) of the low half-wave with rowof(t, 1) of the high one; A is the streamed tile read
//     at [rowof(t, l >> 5)][32 i + (l & 31)].  The weights never go to LDS.
// The MFMA's internal order of its two products is the hardware's; outside it the ORDER is: a score takes one multiply by scale after
// the product; per streamed tile m' = max(m, tile max), r = (m == m') ? 1 : expf(m - m'), x = expf(s - m'), the tile's sum is the
// lane's 16 terms ascending plus the other half-wave's, z = z * r + that, N = N * r, then N accumulates in the MFMA; Y = N / z is one
// IEEE division.  Backward: alpha = expf(s - m) / z (one expf, one division), ds = alpha * (dP - dot), the sums accumulate in the
// MFMA from +0, dQ and dK take one multiply by scale, beta = 1 is one add of the old value.
// Every loop is bounded by n_seg or by a segment length clipped to [0, n_rows].
#include "gnnx_segment_tiles.h"   // the tile copy, the operand readers, rowof and the store of a lane's own row

#pragma clang fp contract(off)

using namespace gnnx;
using namespace gnnx::seg;

namespace {

struct Args {
    int32_t n_seg, n_rows, H, D;
    const int32_t *segptr;
    float scale;
    const float *Q, *K, *V, *G, *Yin;
    int64_t ldq, ldk, ldv, ldg, ldyin;
    const float *rowmax, *rowsum, *dot;        // backward inputs, [n_rows, H] (dot: column side)
    float *rowmax_out, *rowsum_out, *dot_out;  // forward outputs; row side: dot
    float *A, *B;                              // forward: Y; row side: dQ; column side: dV, dK
    int64_t lda, ldb;
    int beta;
};

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int DP, bool VEC>
__global__ __launch_bounds__(kWave) void fwd_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) float ks[Lds<DP>::kFloats], vs[Lds<DP>::kFloats];
    const int lane = threadIdx.x, hf = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kTile, r1 = r0 + kTile < a.n_rows ? r0 + kTile : a.n_rows;
    const int64_t row = r0 + (lane & 31);
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    copy_in<DP, VEC>(ks, a.Q, a.ldq, c0, a.D, r0, r1, lane);
    __syncthreads();
    float q[DP / 2];
    own_regs<DP>(ks, q, lane);
    __syncthreads();

    f32x16 N[blocks_of<DP>()];
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) N[i][r] = 0.f;
    float m = -INFINITY, z = 0.f;

    for_segments(a.segptr, a.n_seg, a.n_rows, r0, r1, row, [&](int64_t lo, int64_t hi, bool active) {
        for (int64_t kb = lo; kb < hi; kb += kTile) {
            copy_in<DP, VEC>(ks, a.K, a.ldk, c0, a.D, kb, hi, lane);
            copy_in<DP, VEC>(vs, a.V, a.ldv, c0, a.D, kb, hi, lane);
            __syncthreads();
            f32x16 s = score_like<DP>(ks, q, lane);
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[r] = (active && kb + rowof(r, hf) < hi) ? a.scale * s[r] : -INFINITY;
                tmax = fmaxf(tmax, s[r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
            const float m_new = active ? fmaxf(m, tmax) : m;
            const float rs = active ? rescale_of(m, m_new) : 1.f;
            float zt = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[r] = active ? expf(s[r] - m_new) : 0.f;   // a masked key: expf(-inf) = +0
                zt = zt + s[r];
            }
            zt = zt + __shfl_xor(zt, 32, kWave);
            z = z * rs + zt;
            m = m_new;
#pragma unroll
            for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
                for (int r = 0; r < 16; r++) N[i][r] = N[i][r] * rs;
            out_like<DP>(vs, s, N, lane);
            __syncthreads();
        }
    });

    if (row >= r1) return;
    const bool some = z > 0.f;   // a row that no segment holds: Y = +0, m = -inf, z = +0
    store_own<DP, VEC>(N, a.A, a.lda, row, c0, a.D, lane, [&](float n, const float *) { return some ? __fdiv_rn(n, z) : 0.f; });
    if (hf == 0) {
        if (a.rowmax_out) a.rowmax_out[row * a.H + h] = m;
        if (a.rowsum_out) a.rowsum_out[row * a.H + h] = z;
    }
}

// ---- backward, row side ----------------------------------------------------------------------------------------------------------
template <int DP, bool VEC>
__global__ __launch_bounds__(kWave) void bwd_rows_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) float ks[Lds<DP>::kFloats], vs[Lds<DP>::kFloats];
    const int lane = threadIdx.x, hf = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kTile, r1 = r0 + kTile < a.n_rows ? r0 + kTile : a.n_rows;
    const int64_t row = r0 + (lane & 31);
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    copy_in<DP, VEC>(ks, a.Q, a.ldq, c0, a.D, r0, r1, lane);
    copy_in<DP, VEC>(vs, a.G, a.ldg, c0, a.D, r0, r1, lane);
    __syncthreads();
    float q[DP / 2], g[DP / 2];
    own_regs<DP>(ks, q, lane);
    own_regs<DP>(vs, g, lane);
    __syncthreads();
    copy_in<DP, VEC>(ks, a.Yin, a.ldyin, c0, a.D, r0, r1, lane);
    __syncthreads();
    float dot = 0.f;
    {
        float y[DP / 2];
        own_regs<DP>(ks, y, lane);
#pragma unroll
        for (int k = 0; k < DP / 2; k++) dot = dot + g[k] * y[k];
        dot = dot + __shfl_xor(dot, 32, kWave);
    }
    __syncthreads();
    const bool mine = row < r1;
    if (mine && hf == 0) a.dot_out[row * a.H + h] = dot;
    const float m = mine ? a.rowmax[row * a.H + h] : 0.f, z = mine ? a.rowsum[row * a.H + h] : 1.f;

    f32x16 dq[blocks_of<DP>()];
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) dq[i][r] = 0.f;

    for_segments(a.segptr, a.n_seg, a.n_rows, r0, r1, row, [&](int64_t lo, int64_t hi, bool active) {
        for (int64_t kb = lo; kb < hi; kb += kTile) {
            copy_in<DP, VEC>(ks, a.K, a.ldk, c0, a.D, kb, hi, lane);
            copy_in<DP, VEC>(vs, a.V, a.ldv, c0, a.D, kb, hi, lane);
            __syncthreads();
            f32x16 s = score_like<DP>(ks, q, lane);
            const f32x16 dp = score_like<DP>(vs, g, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool valid = active && kb + rowof(r, hf) < hi;
                const float al = __fdiv_rn(expf(a.scale * s[r] - m), z);
                s[r] = valid ? al * (dp[r] - dot) : 0.f;
            }
            out_like<DP>(ks, s, dq, lane);
            __syncthreads();
        }
    });

    if (!mine) return;
    store_own<DP, VEC>(dq, a.A, a.lda, row, c0, a.D, lane, [&](float v, const float *) { return a.scale * v; });
}

// ---- backward, column side ---------------------------------------------------------------------------------------------------------
template <int DP, bool VEC>
__global__ __launch_bounds__(kWave) void bwd_cols_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) float qs[Lds<DP>::kFloats], gs[Lds<DP>::kFloats];
    __shared__ float st_m[kTile], st_z[kTile], st_d[kTile];
    const int lane = threadIdx.x, hf = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kTile, r1 = r0 + kTile < a.n_rows ? r0 + kTile : a.n_rows;
    const int64_t row = r0 + (lane & 31);   // the lane's own KEY
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    copy_in<DP, VEC>(qs, a.K, a.ldk, c0, a.D, r0, r1, lane);
    copy_in<DP, VEC>(gs, a.V, a.ldv, c0, a.D, r0, r1, lane);
    __syncthreads();
    float k[DP / 2], v[DP / 2];
    own_regs<DP>(qs, k, lane);
    own_regs<DP>(gs, v, lane);
    __syncthreads();

    f32x16 dv[blocks_of<DP>()], dk[blocks_of<DP>()];
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) dv[i][r] = 0.f, dk[i][r] = 0.f;

    for_segments(a.segptr, a.n_seg, a.n_rows, r0, r1, row, [&](int64_t lo, int64_t hi, bool active) {
        for (int64_t qb = lo; qb < hi; qb += kTile) {
            copy_in<DP, VEC>(qs, a.Q, a.ldq, c0, a.D, qb, hi, lane);
            copy_in<DP, VEC>(gs, a.G, a.ldg, c0, a.D, qb, hi, lane);
            if (lane < kTile) {   // a query past the segment's end: finite statistics, its weight is masked below
                const int64_t i = qb + lane;
                const bool ok = i < hi;
                st_m[lane] = ok ? a.rowmax[i * a.H + h] : 0.f;
                st_z[lane] = ok ? a.rowsum[i * a.H + h] : 1.f;
                st_d[lane] = ok ? a.dot[i * a.H + h] : 0.f;
            }
            __syncthreads();
            f32x16 al = score_like<DP>(qs, k, lane);
            f32x16 ds = score_like<DP>(gs, v, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = rowof(r, hf);
                const bool valid = active && qb + i < hi;
                const float w = __fdiv_rn(expf(a.scale * al[r] - st_m[i]), st_z[i]);
                al[r] = valid ? w : 0.f;
                ds[r] = valid ? w * (ds[r] - st_d[i]) : 0.f;
            }
            out_like<DP>(gs, al, dv, lane);
            out_like<DP>(qs, ds, dk, lane);
            __syncthreads();
        }
    });

    if (row >= r1) return;
    const bool add = a.beta != 0;
    store_own<DP, VEC>(dv, a.A, a.lda, row, c0, a.D, lane, [&](float x, const float *old) { return add ? *old + x : x; });
    store_own<DP, VEC>(dk, a.B, a.ldb, row, c0, a.D, lane, [&](float x, const float *old) {
        const float t = a.scale * x;
        return add ? *old + t : t;
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define SEG_ATTN_ONE(kernel, DP)                                                                       \
    do {                                                                                               \
        if (vec) hipLaunchKernelGGL((kernel<DP, true>), grid, dim3(kWave), 0, st, a);                  \
        else hipLaunchKernelGGL((kernel<DP, false>), grid, dim3(kWave), 0, st, a);                     \
    } while (0)

// the instantiation whose padded width holds D, on the 16-byte or the scalar copy path
#define SEG_ATTN_LAUNCH(kernel)                                                                        \
    do {                                                                                               \
        const dim3 grid((uint32_t)ceil_div(a.n_rows, kTile), (uint32_t)a.H);                           \
        hipStream_t st = as_stream(stream);                                                            \
        GNNX_SEG_FOR_DP(a.D, SEG_ATTN_ONE, kernel);                                                    \
        GNNX_LAUNCH_CHECK();                                                                           \
    } while (0)

}  // namespace

GNNX_API int gnnx_segment_attn_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_heads, int32_t head_dim, float scale,
                                   const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv, float *d_Y, int64_t ldy,
                                   float *d_rowmax, float *d_rowsum, void *stream)
{
    const int rc = check_self_attn(n_seg, n_rows, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldq >= F && ldk >= F && ldv >= F && ldy >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    if (n_rows == 0 || n_seg == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_Q && d_K && d_V && d_Y && d_rowmax && d_rowsum, GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.scale = scale;
    a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.A = d_Y, a.lda = ldy, a.rowmax_out = d_rowmax, a.rowsum_out = d_rowsum;
    const bool vec = head_dim % 4 == 0 && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(ldy, d_Y);
    SEG_ATTN_LAUNCH(fwd_kernel);
    return GNNX_OK;
}

GNNX_API int gnnx_segment_attn_bwd_rows_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_heads, int32_t head_dim, float scale,
                                            const float *d_G, int64_t ldg, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                                            const float *d_V, int64_t ldv, const float *d_Y, int64_t ldy, const float *d_rowmax,
                                            const float *d_rowsum, float *d_dQ, int64_t lddq, float *d_dot, void *stream)
{
    const int rc = check_self_attn(n_seg, n_rows, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && ldy >= F && lddq >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    if (n_rows == 0 || n_seg == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_G && d_Q && d_K && d_V && d_Y && d_rowmax && d_rowsum && d_dQ && d_dot, GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.scale = scale;
    a.G = d_G, a.ldg = ldg, a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.Yin = d_Y, a.ldyin = ldy;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.A = d_dQ, a.lda = lddq, a.dot_out = d_dot;
    const bool vec = head_dim % 4 == 0 && vec4(ldg, d_G) && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(ldy, d_Y) && vec4(lddq, d_dQ);
    SEG_ATTN_LAUNCH(bwd_rows_kernel);
    return GNNX_OK;
}

GNNX_API int gnnx_segment_attn_bwd_cols_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_heads, int32_t head_dim, float scale,
                                            const float *d_G, int64_t ldg, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                                            const float *d_V, int64_t ldv, const float *d_rowmax, const float *d_rowsum, const float *d_dot,
                                            float beta, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, void *stream)
{
    const int rc = check_self_attn(n_seg, n_rows, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && lddk >= F && lddv >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    if (n_rows == 0 || n_seg == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_G && d_Q && d_K && d_V && d_rowmax && d_rowsum && d_dot && d_dK && d_dV, GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.scale = scale;
    a.G = d_G, a.ldg = ldg, a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot = d_dot, a.A = d_dV, a.lda = lddv, a.B = d_dK, a.ldb = lddk, a.beta = beta != 0.f;
    const bool vec = head_dim % 4 == 0 && vec4(ldg, d_G) && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(lddk, d_dK) && vec4(lddv, d_dV);
    SEG_ATTN_LAUNCH(bwd_cols_kernel);
    return GNNX_OK;
}
