// Negative sampling off a CSR and the rank counts of link evaluation -- include/gnnx.h "negative sampling, ranking".
//   * negatives: draw t of entry j of row i of the positives is the r-th smallest column that row i of the excluded pattern does not
//     hold, r = floor(h * count / 2^64) with h a SplitMix64 key of (seed, i, j, t).  The r-th non-member is found without a list of
//     non-members: for the row's ascending columns c_x, g(x) = c_x - x is non-decreasing, J(r) = #{x : g(x) <= r} is one upper-bound
//     search and the answer is r + J(r) (the self column, when it is excluded and not stored, shifts r by one past it).  Work is dealt
//     in the ENTRY domain, as gnnx_sddmm.hip deals it: a wavefront owns kRun consecutive positives and finds the rows of its first and
//     last one in rowptr_pos (two wave-uniform searches); the run's (positive, draw) items go to the lanes draw-fastest, so the m draws
//     of a positive sit on adjacent lanes, search the same row and share the loads of the search's top levels.  A lane finds its
//     positive's row between the run's two rows.  Hub rows spread over the device and need no plan.
//   * rank counts: a lane group of 1 .. 64 lanes (by m) per positive streams its m negative scores once and sums three integers.
// Integer work, 64-bit offsets.  Every loop is a binary search or bounded by m; there is no rejection loop and no spin wait.  The one
// atomic is the counter of unfilled draws.
#include "gnnx_common.h"
#include "gnnx_rng.h"

using namespace gnnx;

namespace {

constexpr int kRun = GNNX_NEG_RUN;   // consecutive positives of one wavefront
constexpr uint64_t kDomain = 0x6E65676174697665ull;   // "negative": the draw is independent of the neighbour sampler's under one seed

// the smallest row r of lo .. hi with rowptr[r + 1] > p: the row that stores entry p when it lies in lo .. hi, empty rows skipped
__device__ __forceinline__ int32_t row_between(const int32_t *rowptr, int32_t lo, int32_t hi, int64_t p)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)rowptr[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

struct Args {
    int32_t n_rows, n_cols, m;
    uint32_t flags;
    int64_t nnz_pos;
    uint64_t s;   // splitmix64(seed ^ kDomain)
    const int32_t *rowptr_pos, *rowptr_ex, *colidx_ex;
    int32_t *neg, *unfilled;
};

// J(r) = #{x < d : c[x] - x <= r}, searched from `lo` on (J is non-decreasing in r)
__device__ __forceinline__ int64_t members_up_to(const int32_t *c, int64_t lo, int64_t d, int64_t r)
{
    int64_t hi = d;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)c[mid] - mid <= r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 4 wavefronts per block, kRun positives per wavefront
__global__ __launch_bounds__(256) void negatives_kernel(Args a)
{
    const uint32_t lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kRun;
    if (p0 >= a.nnz_pos) return;
    const int64_t p1 = p0 + kRun < a.nnz_pos ? p0 + kRun : a.nnz_pos;
    const int32_t row_lo = row_between(a.rowptr_pos, 0, a.n_rows - 1, p0);
    const int32_t row_hi = row_between(a.rowptr_pos, row_lo, a.n_rows - 1, p1 - 1);
    const uint32_t m = (uint32_t)a.m;
    // item x = lane, lane + 64, ... of the run is draw x % m of positive p0 + x / m; (dq, t) is carried, not divided out of a 64-bit x
    int64_t dq = lane / m;
    uint32_t t = lane % m;
    for (; p0 + dq < p1; t += 64, dq += t / m, t %= m) {
        const int64_t q = p0 + dq;
        const int32_t i = row_between(a.rowptr_pos, row_lo, row_hi, q);
        const uint64_t j = (uint64_t)(q - a.rowptr_pos[i]);
        const int64_t b = a.rowptr_ex[i];
        int64_t d = (int64_t)a.rowptr_ex[i + 1] - b;
        if (d < 0) d = 0;   // (a rowptr that gnnx_csr_validate would refuse)
        const int32_t *c = a.colidx_ex + b;
        bool skip_self = (a.flags & GNNX_NEG_EXCLUDE_SELF) && i < a.n_cols;
        if (skip_self) {   // i joins E unless the row stores it
            int64_t lo = 0, hi = d;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (c[mid] < i) lo = mid + 1;
                else hi = mid;
            }
            skip_self = !(lo < d && c[lo] == i);
        }
        const int64_t count = (int64_t)a.n_cols - d - (skip_self ? 1 : 0);
        int64_t ans = -1;
        if (count > 0) {
            const uint64_t h = splitmix64(splitmix64(a.s ^ ((((uint64_t)(uint32_t)i << 32) | j) * kGolden)) ^ ((uint64_t)t * kGolden));
            const int64_t r = (int64_t)__umul64hi(h, (uint64_t)count);
            int64_t J = members_up_to(c, 0, d, r);
            ans = r + J;
            if (skip_self && ans >= i) {
                J = members_up_to(c, J, d, r + 1);
                ans = r + 1 + J;
            }
        } else if (t == 0) {
            atomicAdd(a.unfilled, a.m);
        }
        a.neg[q * m + t] = (int32_t)ans;
    }
}

// ---- rank counts -----------------------------------------------------------------------------------------------------------------
// 256 / G positives per block, G lanes per positive
template <int G>
__global__ __launch_bounds__(256) void rank_counts_kernel(int64_t n_pos, int32_t m, const float *__restrict__ s, const float *__restrict__ q,
                                                           const int32_t *__restrict__ neg, int32_t *__restrict__ greater,
                                                           int32_t *__restrict__ equal, int32_t *__restrict__ valid)
{
    const int l = threadIdx.x % G;
    const int64_t p = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (p >= n_pos) return;   // uniform in the lane group; shuffles below only ever meet lanes of the own group
    const float sp = s[p];
    const int64_t base = p * m;
    int32_t g = 0, e = 0, below = 0;
    for (int32_t t = l; t < m; t += G) {
        if (neg && neg[base + t] < 0) continue;
        const float v = q[base + t];
        g += v > sp;
        e += v == sp;
        below += v < sp;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        g += __shfl_xor(g, off, 64);
        e += __shfl_xor(e, off, 64);
        below += __shfl_xor(below, off, 64);
    }
    if (l == 0) {
        greater[p] = g;
        equal[p] = e;
        valid[p] = g + e + below;
    }
}

template <int G>
int launch_rank_counts(int64_t n_pos, int32_t m, const float *s, const float *q, const int32_t *neg, int32_t *greater, int32_t *equal,
                       int32_t *valid, hipStream_t st)
{
    hipLaunchKernelGGL(rank_counts_kernel<G>, dim3((uint32_t)ceil_div(n_pos, 256 / G)), dim3(256), 0, st, n_pos, m, s, q, neg, greater, equal, valid);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_csr_sample_negatives(int32_t n_rows, int32_t n_cols, int64_t nnz_pos, const int32_t *d_rowptr_pos, int64_t nnz_ex,
                                       const int32_t *d_rowptr_ex, const int32_t *d_colidx_ex, int32_t m, uint64_t seed, uint32_t flags,
                                       int32_t *d_neg, int64_t *n_unfilled_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz_pos >= 0 && nnz_ex >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(m >= 1, GNNX_ERR_INVALID_ARG, "the number of negatives per positive must be at least 1, got %d", m);
    GNNX_REQUIRE(nnz_pos < (1ll << 31) && nnz_pos * m < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz_pos * m does not fit the int32 entry index");
    GNNX_REQUIRE(nnz_ex < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz_ex does not fit the int32 CSR");
    GNNX_REQUIRE(d_rowptr_pos && d_rowptr_ex && n_unfilled_out && (d_neg || nnz_pos == 0) && (d_colidx_ex || nnz_ex == 0), GNNX_ERR_INVALID_ARG,
                 "null pointer");
    GNNX_REQUIRE(d_workspace && workspace_bytes >= GNNX_NEG_WORKSPACE_BYTES, GNNX_ERR_WORKSPACE, "workspace %zu < required %d", workspace_bytes,
                 GNNX_NEG_WORKSPACE_BYTES);
    *n_unfilled_out = 0;
    if (n_rows == 0 || nnz_pos == 0) return GNNX_OK;
    hipStream_t st = as_stream(stream);
    int32_t *counter = reinterpret_cast<int32_t *>((reinterpret_cast<uintptr_t>(d_workspace) + 3u) & ~(uintptr_t)3u);
    const Args a{n_rows, n_cols, m, flags, nnz_pos, splitmix64(seed ^ kDomain), d_rowptr_pos, d_rowptr_ex, d_colidx_ex, d_neg, counter};
    GNNX_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(negatives_kernel, dim3((uint32_t)ceil_div(ceil_div(nnz_pos, kRun), 4)), dim3(256), 0, st, a);
    GNNX_LAUNCH_CHECK();
    int32_t unfilled = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&unfilled, counter, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    *n_unfilled_out = unfilled;
    return GNNX_OK;
}

GNNX_API int gnnx_rank_counts_f32(int64_t n_pos, int32_t m, const float *d_pos_scores, const float *d_neg_scores, const int32_t *d_neg,
                                  int32_t *d_greater, int32_t *d_equal, int32_t *d_valid, void *stream)
{
    GNNX_REQUIRE(n_pos >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_pos < (1ll << 31), GNNX_ERR_INVALID_ARG, "n_pos does not fit int32");
    GNNX_REQUIRE(m >= 1, GNNX_ERR_INVALID_ARG, "the number of negatives per positive must be at least 1, got %d", m);
    if (n_pos == 0) return GNNX_OK;
    GNNX_REQUIRE(d_pos_scores && d_neg_scores && d_greater && d_equal && d_valid, GNNX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = as_stream(stream);
#define GNNX_RANK(G) return launch_rank_counts<G>(n_pos, m, d_pos_scores, d_neg_scores, d_neg, d_greater, d_equal, d_valid, st)
    if (m <= 1) GNNX_RANK(1);
    if (m <= 2) GNNX_RANK(2);
    if (m <= 4) GNNX_RANK(4);
    if (m <= 8) GNNX_RANK(8);
    if (m <= 16) GNNX_RANK(16);
    if (m <= 32) GNNX_RANK(32);
    GNNX_RANK(64);
#undef GNNX_RANK
}
