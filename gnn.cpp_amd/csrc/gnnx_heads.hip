// Multi-head aggregation, edge scores and per-head row sums on a CSR pattern -- include/gnnx.h "multi-head attention".
//   Y[i, h D + j]   = beta Y + (sum_{p in row i, DESCENDING} vals[p ldv + h] * X[c_p, h D + j]) + bias[h D + j]     (aggregation)
//   out[p ldo + h]  = <L[i, h D .. h D + D - 1], R[c_p, h D .. h D + D - 1]>                                         (scores)
// Head h of either result carries the bits of the single-head call (gnnx_spmm.hip, gnnx_sddmm.hip) on slab h of the feature matrices
// and column h of the per-entry arrays: one accumulator per output element in descending column order; the SDDMM lane-group order
// with F := D.  What is new is the shape of the memory traffic: the pattern is read ONCE for all heads, a gathered row is one
// contiguous piece of H D floats (8 heads of 8 features: a 256-byte row instead of eight 32-byte slices), and an entry's H values
// are one contiguous piece.
//   aggregation: G lanes per row, lane l owns features f0 .. f0 + VEC - 1 of tile blockIdx.y and reads the value of head f0 / D.  The
//     group fetches G column indices with one coalesced load and hands them out by shuffle; four neighbour rows and their values are
//     requested before the first is added.  A row is ONE lane group's chain whatever its length (no plan).
//   scores: work is dealt in the non-zero domain as in gnnx_sddmm.hip; GE lanes per entry hold HP = GE / G heads of G lanes each, a
//     pattern with more heads than that takes several passes over the same entry.
#include "gnnx_edge_dot.h"
#include "gnnx_lanes.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

// ---- aggregation ---------------------------------------------------------------------------------------------------------------
struct AggArgs {
    int32_t n_rows, H, D;
    const int32_t *rowptr, *colidx;
    const float *vals;
    int64_t ldv;
    const float *bias, *X;
    int64_t ldx;
    int beta, relu_out;
    float *Y;
    int64_t ldy;
};

__device__ __forceinline__ float mul_add(float acc, float x, float v) { return acc + (x * v); }   // the product rounded, then the sum
__device__ __forceinline__ float4 mul_add(float4 acc, float4 x, float v)
{
    return make_float4(acc.x + (x.x * v), acc.y + (x.y * v), acc.z + (x.z * v), acc.w + (x.w * v));
}
__device__ __forceinline__ float relu(float a) { return a > 0.f ? a : 0.f; }
__device__ __forceinline__ float4 relu(float4 a) { return make_float4(relu(a.x), relu(a.y), relu(a.z), relu(a.w)); }

// B neighbours k .. k + B - 1 from the top of the group's current window (entries top - k, top - k - 1, ...): all loads, then the adds
template <int G, int VEC, int B>
__device__ __forceinline__ void agg_batch(typename Piece<VEC>::F &acc, int k, int32_t top, int32_t myc, int gbase, const float *xf,
                                          const float *vf, const AggArgs &a)
{
    using V = typename Piece<VEC>::F;
    int32_t c[B];
    V x[B];
    float v[B];
#pragma unroll
    for (int u = 0; u < B; u++) c[u] = __shfl(myc, gbase + k + u, 64);
#pragma unroll
    for (int u = 0; u < B; u++) {
        x[u] = *reinterpret_cast<const V *>(xf + (int64_t)c[u] * a.ldx);
        v[u] = vf[(int64_t)(top - k - u) * a.ldv];
    }
#pragma unroll
    for (int u = 0; u < B; u++) acc = mul_add(acc, x[u], v[u]);
}

// grid.x: blocks of 256 / G rows; grid.y: tiles of G * VEC features
template <int G, int VEC>
__global__ __launch_bounds__(256) void agg_heads_kernel(AggArgs a)
{
    using V = typename Piece<VEC>::F;
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) - li;
    const int64_t F = (int64_t)a.H * a.D;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    const bool active = f0 < F;                 // VEC == 4: F % 4 == 0, so the whole piece is inside the row
    const int64_t fa = active ? f0 : 0;         // lanes past the row read feature 0 and never store
    const float *xf = a.X + fa;
    const float *vf = a.vals + fa / a.D;        // the lane's head

    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (row >= a.n_rows) return;                // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int32_t b = a.rowptr[row], e = a.rowptr[row + 1];
    V acc;
    clear(acc);
    for (int32_t hi = e; hi > b; hi -= G) {
        int32_t q = hi - 1 - li;
        q = q >= b ? q : b;
        const int32_t myc = a.colidx[q];
        const int n = hi - b < G ? hi - b : G;
        int k = 0;
        for (; k + 4 <= n; k += 4) agg_batch<G, VEC, 4>(acc, k, hi - 1, myc, gbase, xf, vf, a);
        for (; k < n; k++) agg_batch<G, VEC, 1>(acc, k, hi - 1, myc, gbase, xf, vf, a);
    }
    if (!active) return;
    if (a.bias) acc = add(acc, *reinterpret_cast<const V *>(a.bias + f0));
    V *dst = reinterpret_cast<V *>(a.Y + row * a.ldy + f0);
    if (a.beta) acc = add(*dst, acc);
    if (a.relu_out) acc = relu(acc);
    *dst = acc;
}

template <int G>
int launch_agg(bool vec, const AggArgs &a, int64_t tiles, hipStream_t st)
{
    const dim3 grid((uint32_t)ceil_div(a.n_rows, 256 / G), (uint32_t)tiles);
    if (vec) hipLaunchKernelGGL((agg_heads_kernel<G, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((agg_heads_kernel<G, 1>), grid, dim3(256), 0, st, a);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

// ---- per-head row sums of a per-entry array -------------------------------------------------------------------------------------
// a thread per (row, head): neighbouring lanes read the neighbouring heads of one entry; one accumulator, entries ascending
__global__ __launch_bounds__(256) void rowsum_heads_kernel(const int32_t *__restrict__ rowptr, const float *__restrict__ vals, int64_t ldv,
                                                           int32_t n_rows, int32_t H, float *__restrict__ out, int64_t ldo)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n_rows * H) return;
    const int64_t row = idx / H;
    const int32_t h = (int32_t)(idx - row * H);
    const int32_t b = rowptr[row], e = rowptr[row + 1];
    float acc = 0.f;
    for (int64_t p = b; p < e; p++) acc = acc + vals[p * ldv + h];
    out[row * ldo + h] = acc;
}

// ---- scores (the dot product's steps: gnnx_edge_dot.h, with F := D on a head's slab) --------------------------------------------
struct ScoreArgs {
    int32_t n_rows, H, D;
    int64_t nnz;
    const int32_t *rowptr, *colidx;
    const float *L;
    int64_t ldl;
    const float *R;
    int64_t ldr;
    float *out;
    int64_t ldo;
    int32_t GE, HP;   // lanes per entry (a power of two, G <= GE <= 64) and heads per pass = GE / G
};

// G lanes per head (the SDDMM lane group of F = D).  FAST: every head fits one pass and every lane owns at most one chunk (D <= 256):
// the L piece stays in a register until the row changes and kInFlight R pieces are in flight.
template <int G, bool VEC, bool FAST>
__global__ __launch_bounds__(256) void score_heads_kernel(ScoreArgs a)
{
    const int32_t Q = (a.D + 3) >> 2;
    const int l = threadIdx.x & (a.GE - 1);
    const int lh = l & (G - 1);            // lane inside the head's group: owns chunks lh, lh + G, ...
    const int hs = l / G;                  // head slot of the pass
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) / a.GE;
    int64_t p = group * kEntriesPerGroup;
    if (p >= a.nnz) return;                // uniform in the lane group
    const int64_t p_end = p + kEntriesPerGroup < a.nnz ? p + kEntriesPerGroup : a.nnz;
    int32_t row = row_of_entry(a.rowptr, a.n_rows, p);
    int64_t row_end = a.rowptr[row + 1];

    if constexpr (FAST) {
        const bool have = hs < a.H && lh < Q;
        const int64_t off = have ? (int64_t)hs * a.D + 4 * (int64_t)lh : 0;   // the lane's chunk; idle lanes load and add nothing
        float4 lreg = make_float4(0.f, 0.f, 0.f, 0.f);
        auto load_L = [&]() {
            if (have) lreg = load_chunk<VEC>(a.L + (int64_t)row * a.ldl + off, 0, a.D - 4 * lh);
        };
        load_L();
        for (; p < p_end; p += kInFlight) {
            int32_t col[kInFlight];
            float4 rreg[kInFlight];
#pragma unroll
            for (int j = 0; j < kInFlight; j++) col[j] = p + j < p_end ? a.colidx[p + j] : -1;
#pragma unroll
            for (int j = 0; j < kInFlight; j++)
                if (col[j] >= 0 && have) rreg[j] = load_chunk<VEC>(a.R + (int64_t)col[j] * a.ldr + off, 0, a.D - 4 * lh);
#pragma unroll
            for (int j = 0; j < kInFlight; j++) {
                if (col[j] < 0) continue;
                if (p + j >= row_end) {
                    while (p + j >= row_end && row + 1 < a.n_rows) {   // the bound holds on a valid CSR; it keeps a bad nnz inside rowptr
                        row++;
                        row_end = a.rowptr[row + 1];
                    }
                    load_L();
                }
                float acc = 0.f;
                if (have) acc = add_chunk<VEC>(acc, lreg, rreg[j], 0, a.D - 4 * lh);
                acc = butterfly<G>(acc);
                if (lh == 0 && hs < a.H) a.out[(p + j) * a.ldo + hs] = acc;
            }
        }
    } else {
        for (; p < p_end; p++) {
            while (p >= row_end && row + 1 < a.n_rows) {
                row++;
                row_end = a.rowptr[row + 1];
            }
            const int32_t c = a.colidx[p];
            const float *lrow = a.L + (int64_t)row * a.ldl, *rrow = a.R + (int64_t)c * a.ldr;
            for (int32_t h0 = 0; h0 < a.H; h0 += a.HP) {   // uniform in the lane group: every lane runs every butterfly
                const int32_t h = h0 + hs;
                float acc = 0.f;
                if (h < a.H) {
                    const float *ls = lrow + (int64_t)h * a.D, *rs = rrow + (int64_t)h * a.D;
                    for (int32_t q = lh; q < Q; q += G) acc = add_chunk<VEC>(acc, load_chunk<VEC>(ls, q, a.D), load_chunk<VEC>(rs, q, a.D), q, a.D);
                }
                acc = butterfly<G>(acc);
                if (lh == 0 && h < a.H) a.out[p * a.ldo + h] = acc;
            }
        }
    }
}

template <int G>
int launch_score(bool vec, ScoreArgs a, hipStream_t st)
{
    int GE = G;
    while (GE < 64 && GE < (int64_t)G * a.H) GE <<= 1;
    a.GE = GE;
    a.HP = GE / G;
    const bool fast = a.HP >= a.H && a.D <= 4 * G;   // one pass, one chunk per lane
    const int64_t blocks = ceil_div(ceil_div(a.nnz, kEntriesPerGroup) * GE, 256);
    GNNX_REQUIRE(blocks < (1ll << 31), GNNX_ERR_UNSUPPORTED, "too many entries for one launch");
    const dim3 grid((uint32_t)blocks);
    if (fast) {
        if (vec) hipLaunchKernelGGL((score_heads_kernel<G, true, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((score_heads_kernel<G, false, true>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((score_heads_kernel<G, true, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((score_heads_kernel<G, false, false>), grid, dim3(256), 0, st, a);
    }
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_spmm_csr_heads_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, const int32_t *d_rowptr,
                                     const int32_t *d_colidx, const float *d_vals, int64_t ldv, const float *d_bias, const float *d_X,
                                     int64_t ldx, float beta, int relu_out, float *d_Y, int64_t ldy, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_heads >= 1 && head_dim >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldv >= n_heads, GNNX_ERR_INVALID_ARG, "ldv < n_heads");
    GNNX_REQUIRE(ldx >= F && ldy >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    if (n_rows == 0) return GNNX_OK;
    GNNX_REQUIRE(d_rowptr && d_colidx && d_vals && d_X && d_Y, GNNX_ERR_INVALID_ARG, "null pointer");
    const bool vec = head_dim % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(d_X) && aligned16(d_Y) && aligned16(d_bias);
    const int64_t lanes = vec ? F / 4 : F;
    const int G = lanes > 32 ? 64 : lanes > 16 ? 32 : lanes > 8 ? 16 : lanes > 4 ? 8 : 4;
    const int64_t tiles = ceil_div(lanes, G);
    GNNX_REQUIRE(tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_heads * head_dim too wide for one launch");
    const AggArgs a{n_rows, n_heads, head_dim, d_rowptr, d_colidx, d_vals, ldv, d_bias, d_X, ldx, beta != 0.f, relu_out != 0, d_Y, ldy};
    hipStream_t st = as_stream(stream);
    switch (G) {
    case 4: return launch_agg<4>(vec, a, tiles, st);
    case 8: return launch_agg<8>(vec, a, tiles, st);
    case 16: return launch_agg<16>(vec, a, tiles, st);
    case 32: return launch_agg<32>(vec, a, tiles, st);
    default: return launch_agg<64>(vec, a, tiles, st);
    }
}

GNNX_API int gnnx_csr_rowsum_heads_f32(const int32_t *d_rowptr, const float *d_vals, int64_t ldv, int32_t n_rows, int32_t n_heads, float *d_out,
                                       int64_t ldo, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_heads >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1");
    GNNX_REQUIRE(ldv >= n_heads && ldo >= n_heads, GNNX_ERR_INVALID_ARG, "ld < n_heads");
    if (n_rows == 0) return GNNX_OK;
    GNNX_REQUIRE(d_rowptr && d_out, GNNX_ERR_INVALID_ARG, "null pointer");   // d_vals may be null on a pattern without entries
    const int64_t blocks = ceil_div((int64_t)n_rows * n_heads, 256);
    GNNX_REQUIRE(blocks < (1ll << 31), GNNX_ERR_UNSUPPORTED, "too many (row, head) pairs for one launch");
    hipLaunchKernelGGL(rowsum_heads_kernel, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), d_rowptr, d_vals, ldv, n_rows, n_heads, d_out,
                       ldo);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_sddmm_csr_heads_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, int64_t nnz, const int32_t *d_rowptr,
                                      const int32_t *d_colidx, const float *d_L, int64_t ldl, const float *d_R, int64_t ldr, float *d_out,
                                      int64_t ldo, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_heads >= 1 && head_dim >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldl >= F && ldr >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(ldo >= n_heads, GNNX_ERR_INVALID_ARG, "ldo < n_heads");
    if (nnz == 0) return GNNX_OK;
    GNNX_REQUIRE(n_rows > 0 && n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    GNNX_REQUIRE(d_rowptr && d_colidx && d_L && d_R && d_out, GNNX_ERR_INVALID_ARG, "null pointer");
    const bool vec = head_dim % 4 == 0 && ldl % 4 == 0 && ldr % 4 == 0 && aligned16(d_L) && aligned16(d_R);
    const ScoreArgs a{n_rows, n_heads, head_dim, nnz, d_rowptr, d_colidx, d_L, ldl, d_R, ldr, d_out, ldo, 0, 0};
    hipStream_t st = as_stream(stream);
    const int32_t Q = (head_dim + 3) / 4;
    if (Q <= 1) return launch_score<1>(vec, a, st);
    if (Q <= 2) return launch_score<2>(vec, a, st);
    if (Q <= 4) return launch_score<4>(vec, a, st);
    if (Q <= 8) return launch_score<8>(vec, a, st);
    if (Q <= 16) return launch_score<16>(vec, a, st);
    if (Q <= 32) return launch_score<32>(vec, a, st);
    return launch_score<64>(vec, a, st);
}
