// Dense CROSS attention between two segment sets of a batch (a few learned query rows per graph attend over that graph's vertices: the
// attention readout, Set Transformer's PMA) -- include/gnnx.h "cross segment attention".  Query row i of query segment
// g = [qsegptr[g], qsegptr[g+1]), key rows j of key segment g = [segptr[g], segptr[g+1]), head h of width D:
//   s_ij = scale * <Q_i, K_j>_h;  m_i = max_j s_ij;  x_ij = expf(s_ij - m_i);  z_i = sum_j x_ij
//   forward    Y_i = (sum_j x_ij V_j) / z_i,  rowmax = m,  rowsum = z
//   bwd, rows  dot[i, h] = <G_i, Y_i>_h;  dQ_i = scale * sum_j ds_ij K_j
//   bwd, cols  dV_j (+)= sum_i alpha_ij G_i;  dK_j (+)= scale * sum_i ds_ij Q_i
// with alpha_ij = x_ij / z_i and ds_ij = alpha_ij (<G_i, V_j>_h - dot[i, h]).  No index array, no workspace, no atomics.
//
// WORK SPLIT, made for FEW queries and MANY keys.
//   Forward and row side: grid = (tiles of T consecutive QUERY rows of the whole batch) x heads, a workgroup of FOUR wavefronts; T = 32,
//   or the smaller power of two that own_rows() picks when 32 would leave the device idle (few queries in all).  The workgroup finds the first segment that holds a query of its tile by binary search in qsegptr and walks the segments that intersect
//   the tile in order; segment g's keys are cut into tiles of 32 from segptr[g].  The (segment, key tile) pairs are numbered as they are
//   walked, t = 0, 1, 2, ..., and pair t belongs to wavefront t & 3: a long graph's keys are spread over the workgroup, and a tile of 32
//   one-query graphs with short key lists spreads the graphs.  Each wavefront keeps its own online (m, z, N) of every own row -- the row
//   side its own dQ partial -- over the pairs it was dealt, by the arithmetic of gnnx_segment_attn.hip, and stages its key tiles in its
//   OWN LDS region: the key loop has no workgroup barrier.  The workgroup's barriers stand around the own-tile load (wavefront 0 copies Q,
//   1 copies G, 2 copies Y; every wavefront reads them into registers) and around the merge.
//   MERGE, through LDS, one thread per (own row, 4 features), in ascending wavefront order:
//     m* = max(max(max(m_0, m_1), m_2), m_3);   r_w = (m_w == m*) ? 1 : expf(m_w - m*);
//     z = ((z_0 r_0 + z_1 r_1) + z_2 r_2) + z_3 r_3;   N likewise, element by element;   Y = N / z, one IEEE division.
//   A wavefront that saw no key of a row holds (m, z, N) = (-inf, +0, +0): its r is expf(-inf) = +0, or 1 when no wavefront saw one
//   (-inf == -inf), never expf(-inf - -inf).  z == 0 after the merge -- an empty key segment, a query no segment holds -- writes Y = +0.
//   Row side: dQ = scale * (((p_0 + p_1) + p_2) + p_3) of the four partials.
//   Column side: grid = (tiles of 32 consecutive KEY rows) x heads, ONE wavefront per workgroup, as gnnx_segment_attn.hip's: it walks the
//   key segments that intersect its tile and streams the QUERIES of those segments (few: nothing to split), one accumulator per element.
//
// LDS.  A wavefront's region is two [32][DP + 4] tiles (keys and values), 256 (DP + 4) bytes; the workgroup's four regions are
// 1024 (DP + 4) bytes: 20 480 / 36 864 / 69 632 / 135 168 for DP = 16 / 32 / 64 / 128 -- dynamic LDS, opted in and checked against the
// device per kernel (lds_opt_in).  The merge reuses a region as [DP][33] partials and 64 statistics (33 DP + 64 <= 64 (DP + 4) floats).
// The column side's two tiles are static LDS (at most 33 792 bytes).
//
// The MFMA arrangement, the tile copy and the operand readers are gnnx_segment_tiles.h's.  Every loop is bounded by n_seg or by a segment
// length clipped to [0, n_q] or [0, n_rows]; a row outside those ranges is never addressed.
#include "gnnx_segment_tiles.h"

#pragma clang fp contract(off)

using namespace gnnx;
using namespace gnnx::seg;

namespace {

constexpr int kWaves = 4;          // wavefronts of a forward / row-side workgroup
constexpr int kMergePitch = 33;    // the merge's [DP][33] partials: a wavefront's 32 rows of two feature groups fall on distinct banks

struct Args {
    int32_t n_seg, n_rows, n_q, H, D;
    int32_t own;                               // forward and row side: the queries of a workgroup's own tile, own_rows()
    const int32_t *segptr, *qsegptr;
    float scale;
    const float *Q, *K, *V, *G, *Yin;
    int64_t ldq, ldk, ldv, ldg, ldyin;
    const float *rowmax, *rowsum, *dot;        // backward inputs, [n_q, H] (dot: column side)
    float *rowmax_out, *rowsum_out, *dot_out;  // forward outputs; row side: dot
    float *A, *B;                              // forward: Y; row side: dQ; column side: dV, dK
    int64_t lda, ldb;
    int beta;
};

template <int DP> constexpr size_t lds_bytes() { return (size_t)kWaves * 2 * Lds<DP>::kFloats * sizeof(float); }

// what __syncthreads is to a workgroup, for the lanes of ONE wavefront and its own LDS region
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int64_t clip(int64_t v, int64_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// body(klo, khi, active) for every segment with queries in the tile [r0, r1) and a non-empty key range [klo, khi); active: the lane's own
// query is in the segment
template <class Body>
__device__ __forceinline__ void for_query_segments(const Args &a, int64_t r0, int64_t r1, int64_t row, Body body)
{
    for (int32_t g = first_segment(a.qsegptr, a.n_seg, r0); g < a.n_seg; g++) {
        if (a.qsegptr[g] >= r1) break;
        const int64_t qlo = clip(a.qsegptr[g], a.n_q), qhi = clip(a.qsegptr[g + 1], a.n_q);
        const int64_t klo = clip(a.segptr[g], a.n_rows), khi = clip(a.segptr[g + 1], a.n_rows);
        if (qhi > qlo && khi > klo) body(klo, khi, row >= qlo && row < qhi && row < r1);
    }
}

// body(kb) for the key tiles of [klo, khi) that the running tile number deals to wavefront w; t (mod 4) moves past the segment
template <class Body>
__device__ __forceinline__ void for_dealt_tiles(int64_t klo, int64_t khi, int w, int &t, Body body)
{
    const int64_t n_tiles = (khi - klo + kTile - 1) / kTile;
    for (int64_t j = (w - t) & (kWaves - 1); j < n_tiles; j += kWaves) body(klo + j * kTile);
    t = (int)((t + n_tiles) & (kWaves - 1));
}

// the wavefront's [feature][own row] accumulators -> its region as [DP][33]
template <int DP>
__device__ __forceinline__ void partial_out(float *region, const f32x16 (&acc)[blocks_of<DP>()], int lane)
{
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = 32 * i + rowof(r, lane >> 5);
            if (f < DP) region[f * kMergePitch + (lane & 31)] = acc[i][r];
        }
}

// v[0..3] -> M[row][col0 + d .. d + 3], the columns below D
template <bool VEC>
__device__ __forceinline__ void store4(float *M, int64_t ld, int64_t row, int64_t col0, int d, int32_t D, const float (&v)[4])
{
    float *base = M + row * ld + col0 + d;
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(base) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (d + j < D) base[j] = v[j];
    }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int DP, bool VEC>
__global__ __launch_bounds__(kWaves *kWave) void cross_fwd_kernel(Args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kRegion = 2 * Lds<DP>::kFloats;
    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave, hf = lane >> 5;
    float *ks = lds + w * kRegion, *vs = ks + Lds<DP>::kFloats;
    const int64_t r0 = (int64_t)blockIdx.x * a.own, r1 = r0 + a.own < a.n_q ? r0 + a.own : a.n_q;
    const int64_t row = r0 + (lane & 31);
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    if (w == 0) copy_in<DP, VEC>(lds, a.Q, a.ldq, c0, a.D, r0, r1, lane);
    __syncthreads();
    float q[DP / 2];
    own_regs<DP>(lds, q, lane);
    __syncthreads();

    f32x16 N[blocks_of<DP>()];
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) N[i][r] = 0.f;
    float m = -INFINITY, z = 0.f;

    int t = 0;
    for_query_segments(a, r0, r1, row, [&](int64_t klo, int64_t khi, bool active) {
        for_dealt_tiles(klo, khi, w, t, [&](int64_t kb) {
            copy_in<DP, VEC>(ks, a.K, a.ldk, c0, a.D, kb, khi, lane);
            copy_in<DP, VEC>(vs, a.V, a.ldv, c0, a.D, kb, khi, lane);
            wave_sync();
            f32x16 s = score_like<DP>(ks, q, lane);
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[r] = (active && kb + rowof(r, hf) < khi) ? a.scale * s[r] : -INFINITY;
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
            wave_sync();
        });
    });

    // the merge: every wavefront's (m, z, N) into its own region, then one thread per (own row, 4 features)
    partial_out<DP>(ks, N, lane);
    if (hf == 0) ks[DP * kMergePitch + lane] = m, ks[DP * kMergePitch + kTile + lane] = z;
    __syncthreads();
    const int col = threadIdx.x & 31, fg = threadIdx.x >> 5;
    const int64_t orow = r0 + col;
    if (orow >= r1) return;
    float rw[kWaves], ms = -INFINITY, zs = 0.f;
#pragma unroll
    for (int u = 0; u < kWaves; u++) ms = fmaxf(ms, lds[u * kRegion + DP * kMergePitch + col]);
#pragma unroll
    for (int u = 0; u < kWaves; u++) {
        rw[u] = rescale_of(lds[u * kRegion + DP * kMergePitch + col], ms);
        const float zu = lds[u * kRegion + DP * kMergePitch + kTile + col] * rw[u];
        zs = u == 0 ? zu : zs + zu;
    }
    const bool some = zs > 0.f;   // an empty key segment, a query that no segment holds: Y = +0, m = -inf, z = +0
    for (int d = 4 * fg; d < a.D; d += 4 * (kWaves * kWave / kTile)) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float n = 0.f;
#pragma unroll
            for (int u = 0; u < kWaves; u++) {
                const float nu = lds[u * kRegion + (d + j) * kMergePitch + col] * rw[u];
                n = u == 0 ? nu : n + nu;
            }
            v[j] = some ? __fdiv_rn(n, zs) : 0.f;
        }
        store4<VEC>(a.A, a.lda, orow, c0, d, a.D, v);
    }
    if (fg == 0) {
        a.rowmax_out[orow * a.H + h] = ms;
        a.rowsum_out[orow * a.H + h] = zs;
    }
}

// ---- backward, row side ----------------------------------------------------------------------------------------------------------
template <int DP, bool VEC>
__global__ __launch_bounds__(kWaves *kWave) void cross_bwd_rows_kernel(Args a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kRegion = 2 * Lds<DP>::kFloats;
    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave, hf = lane >> 5;
    float *ks = lds + w * kRegion, *vs = ks + Lds<DP>::kFloats;
    const int64_t r0 = (int64_t)blockIdx.x * a.own, r1 = r0 + a.own < a.n_q ? r0 + a.own : a.n_q;
    const int64_t row = r0 + (lane & 31);
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    if (w == 0) copy_in<DP, VEC>(ks, a.Q, a.ldq, c0, a.D, r0, r1, lane);
    if (w == 1) copy_in<DP, VEC>(ks, a.G, a.ldg, c0, a.D, r0, r1, lane);
    if (w == 2) copy_in<DP, VEC>(ks, a.Yin, a.ldyin, c0, a.D, r0, r1, lane);
    __syncthreads();
    float q[DP / 2], g[DP / 2];
    own_regs<DP>(lds, q, lane);
    own_regs<DP>(lds + kRegion, g, lane);
    float dot = 0.f;
    {
        float y[DP / 2];
        own_regs<DP>(lds + 2 * kRegion, y, lane);
#pragma unroll
        for (int k = 0; k < DP / 2; k++) dot = dot + g[k] * y[k];
        dot = dot + __shfl_xor(dot, 32, kWave);
    }
    __syncthreads();
    const bool mine = row < r1;
    if (mine && hf == 0 && w == 0) a.dot_out[row * a.H + h] = dot;
    const float m = mine ? a.rowmax[row * a.H + h] : 0.f, z = mine ? a.rowsum[row * a.H + h] : 1.f;

    f32x16 dq[blocks_of<DP>()];
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) dq[i][r] = 0.f;

    int t = 0;
    for_query_segments(a, r0, r1, row, [&](int64_t klo, int64_t khi, bool active) {
        for_dealt_tiles(klo, khi, w, t, [&](int64_t kb) {
            copy_in<DP, VEC>(ks, a.K, a.ldk, c0, a.D, kb, khi, lane);
            copy_in<DP, VEC>(vs, a.V, a.ldv, c0, a.D, kb, khi, lane);
            wave_sync();
            f32x16 s = score_like<DP>(ks, q, lane);
            const f32x16 dp = score_like<DP>(vs, g, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool valid = active && kb + rowof(r, hf) < khi;
                const float al = __fdiv_rn(expf(a.scale * s[r] - m), z);
                s[r] = valid ? al * (dp[r] - dot) : 0.f;
            }
            out_like<DP>(ks, s, dq, lane);
            wave_sync();
        });
    });

    partial_out<DP>(ks, dq, lane);
    __syncthreads();
    const int col = threadIdx.x & 31, fg = threadIdx.x >> 5;
    const int64_t orow = r0 + col;
    if (orow >= r1) return;
    for (int d = 4 * fg; d < a.D; d += 4 * (kWaves * kWave / kTile)) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float p = lds[(d + j) * kMergePitch + col];
#pragma unroll
            for (int u = 1; u < kWaves; u++) p = p + lds[u * kRegion + (d + j) * kMergePitch + col];
            v[j] = a.scale * p;
        }
        store4<VEC>(a.A, a.lda, orow, c0, d, a.D, v);
    }
}

// ---- backward, column side ---------------------------------------------------------------------------------------------------------
template <int DP, bool VEC>
__global__ __launch_bounds__(kWave) void cross_bwd_cols_kernel(Args a)
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

    // the key segments that intersect the tile; of each, the queries [qlo, qhi)
    for (int32_t g = first_segment(a.segptr, a.n_seg, r0); g < a.n_seg; g++) {
        if (a.segptr[g] >= r1) break;
        const int64_t klo = clip(a.segptr[g], a.n_rows), khi = clip(a.segptr[g + 1], a.n_rows);
        const int64_t qlo = clip(a.qsegptr[g], a.n_q), qhi = clip(a.qsegptr[g + 1], a.n_q);
        if (khi <= klo) continue;
        const bool active = row >= klo && row < khi;
        for (int64_t qb = qlo; qb < qhi; qb += kTile) {
            copy_in<DP, VEC>(qs, a.Q, a.ldq, c0, a.D, qb, qhi, lane);
            copy_in<DP, VEC>(gs, a.G, a.ldg, c0, a.D, qb, qhi, lane);
            if (lane < kTile) {   // a query past the segment's end: finite statistics, its weight is masked below
                const int64_t i = qb + lane;
                const bool ok = i < qhi;
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
                const bool valid = active && qb + i < qhi;
                const float wgt = __fdiv_rn(expf(a.scale * al[r] - st_m[i]), st_z[i]);
                al[r] = valid ? wgt : 0.f;
                ds[r] = valid ? wgt * (ds[r] - st_d[i]) : 0.f;
            }
            out_like<DP>(gs, al, dv, lane);
            out_like<DP>(qs, ds, dk, lane);
            __syncthreads();
        }
    }

    if (row >= r1) return;
    const bool add = a.beta != 0;
    store_own<DP, VEC>(dv, a.A, a.lda, row, c0, a.D, lane, [&](float x, const float *old) { return add ? *old + x : x; });
    store_own<DP, VEC>(dk, a.B, a.ldb, row, c0, a.D, lane, [&](float x, const float *old) {
        const float t = a.scale * x;
        return add ? *old + t : t;
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// what all three calls check before any HIP call
int check_common(int32_t n_seg, int32_t n_rows, int32_t n_q, int32_t H, int32_t D)
{
    GNNX_REQUIRE(n_seg >= 0 && n_rows >= 0 && n_q >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(H >= 1 && D >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(n_seg > 0 || (n_rows == 0 && n_q == 0), GNNX_ERR_INVALID_ARG, "rows without a segment");
    GNNX_REQUIRE(D <= kMaxDim, GNNX_ERR_UNSUPPORTED, "head_dim %d > %d", D, kMaxDim);
    GNNX_REQUIRE(H <= 65535, GNNX_ERR_UNSUPPORTED, "%d heads are too many for one launch", H);
    return GNNX_OK;
}

// The queries of an own tile: 32 (the MFMA's N) where that makes at least kFill workgroups, else the largest power of two below it that
// does, else 1 -- 64 graphs with one query each are 64 workgroups a head, not 2.  The columns of the MFMA past the own queries are idle.  A
// function of (n_q, n_heads) alone, so a problem's bits do not depend on the device.
constexpr int64_t kFill = 2 * kNumCU;
int32_t own_rows(int32_t n_q, int32_t H)
{
    int32_t own = kTile;
    while (own > 1 && ceil_div(n_q, own) * H < kFill) own >>= 1;
    return own;
}

// the four-wavefront kernels: the dynamic-LDS opt-in of the instantiation, checked against the device, then the launch
template <int DP, void (*KERNEL)(Args)>
int launch_wide(const char *what, const Args &a, void *stream)
{
    static std::atomic<uint64_t> done{0};   // one per kernel instantiation
    const int rc = lds_opt_in(KERNEL, lds_bytes<DP>(), done, what);
    if (rc) return rc;
    const dim3 grid((uint32_t)ceil_div(a.n_q, a.own), (uint32_t)a.H);
    hipLaunchKernelGGL(KERNEL, grid, dim3(kWaves * kWave), lds_bytes<DP>(), as_stream(stream), a);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

#define CROSS_WIDE_ONE(kernel, DP)                                                                            \
    return vec ? launch_wide<DP, kernel<DP, true>>(#kernel, a, stream) : launch_wide<DP, kernel<DP, false>>(#kernel, a, stream)

#define CROSS_COLS_ONE(kernel, DP)                                                                            \
    do {                                                                                                      \
        if (vec) hipLaunchKernelGGL((kernel<DP, true>), grid, dim3(kWave), 0, as_stream(stream), a);          \
        else hipLaunchKernelGGL((kernel<DP, false>), grid, dim3(kWave), 0, as_stream(stream), a);             \
    } while (0)

int launch_fwd(const Args &a, bool vec, void *stream)
{
    GNNX_SEG_FOR_DP(a.D, CROSS_WIDE_ONE, cross_fwd_kernel);
}

int launch_rows(const Args &a, bool vec, void *stream)
{
    GNNX_SEG_FOR_DP(a.D, CROSS_WIDE_ONE, cross_bwd_rows_kernel);
}

}  // namespace

GNNX_API int gnnx_segment_cross_attn_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_q, const int32_t *d_qsegptr,
                                         int32_t n_heads, int32_t head_dim, float scale, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                                         const float *d_V, int64_t ldv, float *d_Y, int64_t ldy, float *d_rowmax, float *d_rowsum, void *stream)
{
    const int rc = check_common(n_seg, n_rows, n_q, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldq >= F && ldk >= F && ldv >= F && ldy >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    if (n_q == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_qsegptr && d_Q && d_Y && d_rowmax && d_rowsum && (n_rows == 0 || (d_K && d_V)), GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.n_q = n_q, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.qsegptr = d_qsegptr, a.scale = scale;
    a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.A = d_Y, a.lda = ldy, a.rowmax_out = d_rowmax, a.rowsum_out = d_rowsum;
    a.own = own_rows(n_q, n_heads);
    const bool vec = head_dim % 4 == 0 && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(ldy, d_Y);
    return launch_fwd(a, vec, stream);
}

GNNX_API int gnnx_segment_cross_attn_bwd_rows_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_q, const int32_t *d_qsegptr,
                                                  int32_t n_heads, int32_t head_dim, float scale, const float *d_G, int64_t ldg, const float *d_Q,
                                                  int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv, const float *d_Y,
                                                  int64_t ldy, const float *d_rowmax, const float *d_rowsum, float *d_dQ, int64_t lddq, float *d_dot,
                                                  void *stream)
{
    const int rc = check_common(n_seg, n_rows, n_q, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && ldy >= F && lddq >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    if (n_q == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_qsegptr && d_G && d_Q && d_Y && d_rowmax && d_rowsum && d_dQ && d_dot && (n_rows == 0 || (d_K && d_V)),
                 GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.n_q = n_q, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.qsegptr = d_qsegptr, a.scale = scale;
    a.G = d_G, a.ldg = ldg, a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.Yin = d_Y, a.ldyin = ldy;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.A = d_dQ, a.lda = lddq, a.dot_out = d_dot;
    a.own = own_rows(n_q, n_heads);
    const bool vec = head_dim % 4 == 0 && vec4(ldg, d_G) && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(ldy, d_Y) && vec4(lddq, d_dQ);
    return launch_rows(a, vec, stream);
}

GNNX_API int gnnx_segment_cross_attn_bwd_cols_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_q, const int32_t *d_qsegptr,
                                                  int32_t n_heads, int32_t head_dim, float scale, const float *d_G, int64_t ldg, const float *d_Q,
                                                  int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv, const float *d_rowmax,
                                                  const float *d_rowsum, const float *d_dot, float beta, float *d_dK, int64_t lddk, float *d_dV,
                                                  int64_t lddv, void *stream)
{
    const int rc = check_common(n_seg, n_rows, n_q, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && lddk >= F && lddv >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    if (n_rows == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_qsegptr && d_K && d_V && d_dK && d_dV && (n_q == 0 || (d_G && d_Q && d_rowmax && d_rowsum && d_dot)),
                 GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.n_q = n_q, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.qsegptr = d_qsegptr, a.scale = scale;
    a.G = d_G, a.ldg = ldg, a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot = d_dot, a.A = d_dV, a.lda = lddv, a.B = d_dK, a.ldb = lddk, a.beta = beta != 0.f;
    const bool vec = head_dim % 4 == 0 && vec4(ldg, d_G) && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(lddk, d_dK) && vec4(lddv, d_dV);
    const dim3 grid((uint32_t)ceil_div(n_rows, kTile), (uint32_t)n_heads);
    GNNX_SEG_FOR_DP(a.D, CROSS_COLS_ONE, cross_bwd_cols_kernel);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}
