// Dynamic attention scores (GATv2, Brody et al. 2022) and their backward on a CSR pattern -- include/gnnx.h "dynamic attention scores".
//   out[p ldo + h]  = sum_k a[h D + k] * leaky(L[i, h D + k] + R[c_p, h D + k])                                      (scores)
//   dOwn[i, f]      = beta dOwn + sum_{p in row i, DESCENDING} de[m_p ldd + h] * (u_pf > 0 ? a[f] : a[f] * slope)    (backward)
//   T[i, f]         = sum_{p in row i, DESCENDING} de[m_p ldd + h] * leaky(u_pf),   u_pf = Own[i, f] + Other[c_p, f]
// Both are gather-bound like the aggregation: one H D row of R / Other per stored entry, nothing shared between entries but through the
// caches; no MFMA, no LDS, no atomics.
//   scores: the shape of gnnx_heads.hip's score kernel -- work dealt in the non-zero domain (kEntriesPerGroup entries per lane group, the
//     row by row_of_entry: a hub row spreads over the device), GE lanes per entry hold HP = GE / G heads of G lanes each, the sum in the
//     SDDMM lane-group order of F := D (gnnx_edge_dot.h; the chunk step is add_leaky_chunk).  FAST: the lane's chunks of L and of a stay
//     in registers and kInFlight rows of R are requested before the first is consumed.
//   backward: the shape of gnnx_heads.hip's aggregation -- G lanes per row, lane l owns features f0 .. f0 + VEC - 1 of tile blockIdx.y and
//     reads the gradient of head f0 / D; the group fetches G column indices (and mapped positions) with one coalesced load and hands them
//     out by shuffle; four rows of Other are requested before the first is used; the Own and a pieces stay in registers for the whole
//     row.  A row is ONE lane group's chain whatever its length (no plan).
#include "gnnx_edge_dot.h"
#include "gnnx_lanes.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

// ---- scores ----------------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    int32_t n_rows, H, D;
    int64_t nnz;
    const int32_t *rowptr, *colidx;
    const float *L;
    int64_t ldl;
    const float *R;
    int64_t ldr;
    const float *a;
    float slope;
    float *out;
    int64_t ldo;
    int32_t GE, HP;   // lanes per entry (a power of two, G <= GE <= 64) and heads per pass = GE / G
};

// G lanes per head (the SDDMM lane group of F = D).  FAST: every head fits one pass and every lane owns at most one chunk (D <= 256).
template <int G, bool VEC, bool FAST>
__global__ __launch_bounds__(256) void gatv2_score_kernel(ScoreArgs a)
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
        const int32_t left = a.D - 4 * lh;                                    // features from the chunk's first to the head's end
        float4 lreg = make_float4(0.f, 0.f, 0.f, 0.f), areg = lreg;
        if (have) areg = load_chunk<VEC>(a.a + off, 0, left);                 // loop-invariant: beside the L chunk
        auto load_L = [&]() {
            if (have) lreg = load_chunk<VEC>(a.L + (int64_t)row * a.ldl + off, 0, left);
        };
        load_L();
        for (; p < p_end; p += kInFlight) {
            int32_t col[kInFlight];
            float4 rreg[kInFlight];
#pragma unroll
            for (int j = 0; j < kInFlight; j++) col[j] = p + j < p_end ? a.colidx[p + j] : -1;
#pragma unroll
            for (int j = 0; j < kInFlight; j++)
                if (col[j] >= 0 && have) rreg[j] = load_chunk<VEC>(a.R + (int64_t)col[j] * a.ldr + off, 0, left);
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
                if (have) acc = add_leaky_chunk<VEC>(acc, lreg, rreg[j], areg, a.slope, 0, left);
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
                    const float *ls = lrow + (int64_t)h * a.D, *rs = rrow + (int64_t)h * a.D, *as = a.a + (int64_t)h * a.D;
                    for (int32_t q = lh; q < Q; q += G)
                        acc = add_leaky_chunk<VEC>(acc, load_chunk<VEC>(ls, q, a.D), load_chunk<VEC>(rs, q, a.D), load_chunk<VEC>(as, q, a.D),
                                                   a.slope, q, a.D);
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
        if (vec) hipLaunchKernelGGL((gatv2_score_kernel<G, true, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gatv2_score_kernel<G, false, true>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((gatv2_score_kernel<G, true, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gatv2_score_kernel<G, false, false>), grid, dim3(256), 0, st, a);
    }
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    int32_t n_rows, H, D;
    const int32_t *rowptr, *colidx, *entry_map;
    const float *de;
    int64_t ldd;
    const float *Own;
    int64_t ld_own;
    const float *Other;
    int64_t ld_other;
    const float *a;
    float slope;
    int beta;
    float *dOwn;
    int64_t ld_down;
    float *T;
    int64_t ldt;
};

// w = u > 0 ? a : a * slope, the slope product `as` rounded once per row
__device__ __forceinline__ float weight(float u, float a, float as) { return u > 0.f ? a : as; }
__device__ __forceinline__ float4 weight(float4 u, float4 a, float4 as)
{
    return make_float4(weight(u.x, a.x, as.x), weight(u.y, a.y, as.y), weight(u.z, a.z, as.z), weight(u.w, a.w, as.w));
}

// B neighbours k .. k + B - 1 from the top of the group's current window (entries top - k, top - k - 1, ...): all loads, then the adds
template <int G, int VEC, bool WITH_T, int B>
__device__ __forceinline__ void bwd_batch(typename Piece<VEC>::F &acc, typename Piece<VEC>::F &tacc, int k, int32_t myc, int32_t mym, int gbase,
                                          const typename Piece<VEC>::F &own, const typename Piece<VEC>::F &av, const typename Piece<VEC>::F &as,
                                          const float *of, const float *df, const BwdArgs &a)
{
    using V = typename Piece<VEC>::F;
    int32_t c[B], m[B];
    V x[B];
    float d[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
        c[u] = __shfl(myc, gbase + k + u, 64);
        m[u] = __shfl(mym, gbase + k + u, 64);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
        x[u] = *reinterpret_cast<const V *>(of + (int64_t)c[u] * a.ld_other);
        d[u] = df[(int64_t)m[u] * a.ldd];
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
        const V s = add(own, x[u]);                                          // u = Own + Other: the forward's bits (addition commutes)
        acc = add(acc, mul(weight(s, av, as), d[u]));                        // the product rounded, then the sum
        if constexpr (WITH_T) tacc = add(tacc, mul(leaky(s, a.slope), d[u]));
    }
}

// grid.x: blocks of 256 / G rows; grid.y: tiles of G * VEC features
template <int G, int VEC, bool WITH_T>
__global__ __launch_bounds__(256) void gatv2_bwd_kernel(BwdArgs a)
{
    using V = typename Piece<VEC>::F;
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) - li;
    const int64_t F = (int64_t)a.H * a.D;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    const bool active = f0 < F;                 // VEC == 4: F % 4 == 0, so the whole piece is inside the row
    const int64_t fa = active ? f0 : 0;         // lanes past the row read feature 0 and never store
    const float *of = a.Other + fa;
    const float *df = a.de + fa / a.D;          // the lane's head

    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (row >= a.n_rows) return;                // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int32_t b = a.rowptr[row], e = a.rowptr[row + 1];
    V acc, tacc;
    clear(acc);
    clear(tacc);
    if (e > b) {
        const V own = *reinterpret_cast<const V *>(a.Own + row * a.ld_own + fa);
        const V av = *reinterpret_cast<const V *>(a.a + fa);
        const V as = mul(av, a.slope);
        for (int32_t hi = e; hi > b; hi -= G) {
            int32_t q = hi - 1 - li;
            q = q >= b ? q : b;
            const int32_t myc = a.colidx[q];
            const int32_t mym = a.entry_map ? a.entry_map[q] : q;
            const int n = hi - b < G ? hi - b : G;
            int k = 0;
            for (; k + 4 <= n; k += 4) bwd_batch<G, VEC, WITH_T, 4>(acc, tacc, k, myc, mym, gbase, own, av, as, of, df, a);
            for (; k < n; k++) bwd_batch<G, VEC, WITH_T, 1>(acc, tacc, k, myc, mym, gbase, own, av, as, of, df, a);
        }
    }
    if (!active) return;
    if constexpr (WITH_T) *reinterpret_cast<V *>(a.T + row * a.ldt + f0) = tacc;
    V *dst = reinterpret_cast<V *>(a.dOwn + row * a.ld_down + f0);
    if (a.beta) acc = add(*dst, acc);
    *dst = acc;
}

template <int G>
int launch_bwd(bool vec, const BwdArgs &a, int64_t tiles, hipStream_t st)
{
    const dim3 grid((uint32_t)ceil_div(a.n_rows, 256 / G), (uint32_t)tiles);
    if (a.T) {
        if (vec) hipLaunchKernelGGL((gatv2_bwd_kernel<G, 4, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gatv2_bwd_kernel<G, 1, true>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((gatv2_bwd_kernel<G, 4, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gatv2_bwd_kernel<G, 1, false>), grid, dim3(256), 0, st, a);
    }
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_gatv2_scores_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, int64_t nnz, const int32_t *d_rowptr,
                                       const int32_t *d_colidx, const float *d_L, int64_t ldl, const float *d_R, int64_t ldr, const float *d_a,
                                       float negative_slope, float *d_out, int64_t ldo, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_heads >= 1 && head_dim >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldl >= F && ldr >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(ldo >= n_heads, GNNX_ERR_INVALID_ARG, "ldo < n_heads");
    if (nnz == 0) return GNNX_OK;
    GNNX_REQUIRE(n_rows > 0 && n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    GNNX_REQUIRE(d_rowptr && d_colidx && d_L && d_R && d_a && d_out, GNNX_ERR_INVALID_ARG, "null pointer");
    const bool vec = head_dim % 4 == 0 && ldl % 4 == 0 && ldr % 4 == 0 && aligned16(d_L) && aligned16(d_R) && aligned16(d_a);
    const ScoreArgs a{n_rows, n_heads, head_dim, nnz, d_rowptr, d_colidx, d_L, ldl, d_R, ldr, d_a, negative_slope, d_out, ldo, 0, 0};
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

GNNX_API int gnnx_gatv2_scores_bwd_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, int64_t nnz, const int32_t *d_rowptr,
                                           const int32_t *d_colidx, const float *d_de, int64_t ldd, const int32_t *d_entry_map, const float *d_Own,
                                           int64_t ld_own, const float *d_Other, int64_t ld_other, const float *d_a, float negative_slope, float beta,
                                           float *d_dOwn, int64_t ld_down, float *d_T, int64_t ldt, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_heads >= 1 && head_dim >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ld_own >= F && ld_other >= F && ld_down >= F && (!d_T || ldt >= F), GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(ldd >= n_heads, GNNX_ERR_INVALID_ARG, "ldd < n_heads");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE(nnz == 0 || (n_rows > 0 && n_cols > 0), GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    if (n_rows == 0) return GNNX_OK;
    GNNX_REQUIRE(d_rowptr && d_Own && d_a && d_dOwn, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(nnz == 0 || (d_colidx && d_de && d_Other), GNNX_ERR_INVALID_ARG, "null pointer");   // a pattern without entries reads none
    const bool vec = head_dim % 4 == 0 && ld_own % 4 == 0 && ld_other % 4 == 0 && ld_down % 4 == 0 && (!d_T || ldt % 4 == 0) &&
                     aligned16(d_Own) && aligned16(d_Other) && aligned16(d_a) && aligned16(d_dOwn) && aligned16(d_T);
    const int64_t lanes = vec ? F / 4 : F;
    const int G = lanes > 32 ? 64 : lanes > 16 ? 32 : lanes > 8 ? 16 : lanes > 4 ? 8 : 4;
    const int64_t tiles = ceil_div(lanes, G);
    GNNX_REQUIRE(tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_heads * head_dim too wide for one launch");
    const BwdArgs a{n_rows, n_heads, head_dim, d_rowptr, d_colidx, d_entry_map, d_de, ldd, d_Own, ld_own, d_Other, ld_other, d_a, negative_slope,
                    beta != 0.f, d_dOwn, ld_down, d_T, ldt};
    hipStream_t st = as_stream(stream);
    switch (G) {
    case 4: return launch_bwd<4>(vec, a, tiles, st);
    case 8: return launch_bwd<8>(vec, a, tiles, st);
    case 16: return launch_bwd<16>(vec, a, tiles, st);
    case 32: return launch_bwd<32>(vec, a, tiles, st);
    default: return launch_bwd<64>(vec, a, tiles, st);
    }
}
