// Edge scores on a CSR pattern (SDDMM) and the position map between CSR(A) and CSR(A^T) -- include/gnnx.h "edge scores".
//   out[p] = (<L[i,:], R[c_p,:]> * rowscale[i]) * colscale[c_p]      for entry p of row i
// The dot product's ORDER is part of the contract and a function of F alone: gnnx_edge_dot.h states it and holds its steps.  It is a
// vec4 lane group: F = 256 is a wavefront per entry with one 16-byte load per lane, F = 128 two entries per wavefront.  Rows that fail
// the vec4 conditions take scalar loads with the same feature-to-lane assignment: same bits.
//
// Work is dealt in the NON-ZERO domain: a lane group owns kEntriesPerGroup consecutive entries and finds
// the row of its first one by a search in rowptr, so a hub row spreads over the device without a plan.  The L row stays in
// registers until the row changes; the R rows of four entries are requested before the first of them is used (4 rows in flight
// per lane group, 16 wavefronts per CU: the gather shape of the aggregation).  The butterfly is register shuffles; no LDS.
#include "gnnx_edge_dot.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kMaxBlocks = 16384;      // grid cap of the one-thread-per-entry index kernels (grid stride)

// G lanes per entry, CPL = ceil(Q / G) chunks per lane (1 unless G == 64), the L row's chunks in registers.
template <int G, int CPL, bool VEC>
__global__ __launch_bounds__(256) void sddmm_kernel(int32_t n_rows, int32_t F, int64_t nnz, const int32_t *__restrict__ rowptr,
                                                     const int32_t *__restrict__ colidx, const float *__restrict__ Lm, int64_t ldl,
                                                     const float *__restrict__ Rm, int64_t ldr, const float *__restrict__ rowscale,
                                                     const float *__restrict__ colscale, float *__restrict__ out)
{
    const int32_t Q = (F + 3) >> 2;
    const int l = threadIdx.x & (G - 1);
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    int64_t p = group * kEntriesPerGroup;
    if (p >= nnz) return;   // uniform in the lane group; shuffles below only ever meet lanes of the own group
    const int64_t p_end = p + kEntriesPerGroup < nnz ? p + kEntriesPerGroup : nnz;

    int32_t row = row_of_entry(rowptr, n_rows, p);
    int64_t row_end = rowptr[row + 1];
    float4 lreg[CPL];
    float rs = 1.f;
    auto load_L = [&]() {
        const float *lrow = Lm + (int64_t)row * ldl;
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            const int32_t q = l + c * G;
            lreg[c] = q < Q ? load_chunk<VEC>(lrow, q, F) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (rowscale) rs = rowscale[row];
    };
    load_L();

    int32_t col[kInFlight], col_next[kInFlight];
#pragma unroll
    for (int j = 0; j < kInFlight; j++) col[j] = p + j < p_end ? colidx[p + j] : -1;
    for (; p < p_end; p += kInFlight) {
        float4 rreg[kInFlight][CPL];
        float cs[kInFlight];
#pragma unroll
        for (int j = 0; j < kInFlight; j++) col_next[j] = p + kInFlight + j < p_end ? colidx[p + kInFlight + j] : -1;   // one batch ahead
#pragma unroll
        for (int j = 0; j < kInFlight; j++) {
            if (col[j] < 0) continue;
            const float *rrow = Rm + (int64_t)col[j] * ldr;
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                const int32_t q = l + c * G;
                if (q < Q) rreg[j][c] = load_chunk<VEC>(rrow, q, F);
            }
            cs[j] = colscale ? colscale[col[j]] : 1.f;
        }
#pragma unroll
        for (int j = 0; j < kInFlight; j++) {
            if (col[j] < 0) continue;
            if (p + j >= row_end) {
                while (p + j >= row_end && row + 1 < n_rows) {   // the bound holds on a valid CSR; it keeps a bad nnz inside rowptr
                    row++;
                    row_end = rowptr[row + 1];
                }
                load_L();
            }
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                const int32_t q = l + c * G;
                if (q < Q) acc = add_chunk<VEC>(acc, lreg[c], rreg[j][c], q, F);
            }
            acc = butterfly<G>(acc);
            if (rowscale) acc = acc * rs;
            if (colscale) acc = acc * cs[j];
            if (l == 0) out[p + j] = acc;
        }
#pragma unroll
        for (int j = 0; j < kInFlight; j++) col[j] = col_next[j];
    }
}

// rows of more than 1024 features (more than 4 chunks per lane of a 64-lane group): a wavefront per entry walks both rows
template <bool VEC>
__global__ __launch_bounds__(256) void sddmm_wide_kernel(int32_t n_rows, int32_t F, int64_t nnz, const int32_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ colidx, const float *__restrict__ Lm, int64_t ldl,
                                                          const float *__restrict__ Rm, int64_t ldr, const float *__restrict__ rowscale,
                                                          const float *__restrict__ colscale, float *__restrict__ out)
{
    const int32_t Q = (F + 3) >> 2;
    const int l = threadIdx.x & 63;
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    int64_t p = group * kEntriesPerGroup;
    if (p >= nnz) return;
    const int64_t p_end = p + kEntriesPerGroup < nnz ? p + kEntriesPerGroup : nnz;
    int32_t row = row_of_entry(rowptr, n_rows, p);
    int64_t row_end = rowptr[row + 1];
    for (; p < p_end; p++) {
        while (p >= row_end && row + 1 < n_rows) {
            row++;
            row_end = rowptr[row + 1];
        }
        const int32_t c = colidx[p];
        const float *lrow = Lm + (int64_t)row * ldl, *rrow = Rm + (int64_t)c * ldr;
        float acc = 0.f;
        for (int32_t q = l; q < Q; q += 64) acc = add_chunk<VEC>(acc, load_chunk<VEC>(lrow, q, F), load_chunk<VEC>(rrow, q, F), q, F);
        acc = butterfly<64>(acc);
        if (rowscale) acc = acc * rowscale[row];
        if (colscale) acc = acc * colscale[c];
        if (l == 0) out[p] = acc;
    }
}

template <int G, int CPL>
int launch_sddmm(bool vec, int32_t n_rows, int32_t F, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const float *L, int64_t ldl,
                 const float *R, int64_t ldr, const float *rowscale, const float *colscale, float *out, hipStream_t st)
{
    const int64_t groups = ceil_div(nnz, kEntriesPerGroup);
    const int64_t blocks = ceil_div(groups * G, 256);
    GNNX_REQUIRE(blocks < (1ll << 31), GNNX_ERR_UNSUPPORTED, "too many entries for one launch");
    if (vec)
        hipLaunchKernelGGL((sddmm_kernel<G, CPL, true>), dim3((uint32_t)blocks), dim3(256), 0, st, n_rows, F, nnz, rowptr, colidx, L, ldl, R, ldr,
                           rowscale, colscale, out);
    else
        hipLaunchKernelGGL((sddmm_kernel<G, CPL, false>), dim3((uint32_t)blocks), dim3(256), 0, st, n_rows, F, nnz, rowptr, colidx, L, ldl, R, ldr,
                           rowscale, colscale, out);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

// ---- position map CSR(A^T) -> CSR(A) ------------------------------------------------------------------------------------------
// bad |= 1 when an entry's column does not exceed its predecessor's in the same row (unsorted row or duplicate) or is outside
// [0, n_cols)
__global__ __launch_bounds__(256) void csr_ascending_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int32_t n_rows,
                                                             int32_t n_cols, int64_t nnz, int32_t *bad)
{
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * 256) {
        const int32_t c = colidx[p];
        bool ok = c >= 0 && c < n_cols;
        if (ok && p > 0) {
            const int32_t row = row_of_entry(rowptr, n_rows, p);
            if (p > (int64_t)rowptr[row]) ok = colidx[p - 1] < c;
        }
        if (!ok) atomicOr(bad, 1);
    }
}

// entry q = (c, r) of CSR(A^T): map_t[q] = the position of c in row r of CSR(A) (binary search; -1 and bad |= 2 without a partner)
__global__ __launch_bounds__(256) void transpose_map_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                             const int32_t *__restrict__ rowptr_t, const int32_t *__restrict__ colidx_t, int32_t n_rows,
                                                             int32_t n_cols, int64_t nnz, int32_t *__restrict__ map_t, int32_t *bad)
{
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * 256) {
        const int32_t c = row_of_entry(rowptr_t, n_cols, q);
        const int32_t r = colidx_t[q];
        int64_t found = -1;
        if (r >= 0 && r < n_rows) {
            int64_t lo = rowptr[r], hi = rowptr[r + 1];
            if (lo < 0) lo = 0;
            if (hi > nnz) hi = nnz;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                const int32_t v = colidx[mid];
                if (v < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nnz && lo < (int64_t)rowptr[r + 1] && colidx[lo] == c) found = lo;
        }
        map_t[q] = (int32_t)found;
        if (found < 0) atomicOr(bad, 2);
    }
}

inline uint32_t entry_blocks(int64_t n)
{
    const int64_t b = ceil_div(n, 256);
    return (uint32_t)(b > kMaxBlocks ? kMaxBlocks : b);
}

}  // namespace

GNNX_API int gnnx_sddmm_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                const float *d_L, int64_t ldl, const float *d_R, int64_t ldr, const float *d_rowscale,
                                const float *d_colscale, float *d_out, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_feat >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(ldl >= n_feat && ldr >= n_feat, GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (nnz == 0) return GNNX_OK;
    GNNX_REQUIRE(n_rows > 0 && n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    GNNX_REQUIRE(d_rowptr && d_colidx && d_out, GNNX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = as_stream(stream);
    if (n_feat == 0) {
        GNNX_HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(float) * (size_t)nnz, st));   // the empty sum: +0
        return GNNX_OK;
    }
    GNNX_REQUIRE(d_L && d_R, GNNX_ERR_INVALID_ARG, "null pointer");
    const bool vec = n_feat % 4 == 0 && ldl % 4 == 0 && ldr % 4 == 0 && aligned16(d_L) && aligned16(d_R);
    const int32_t Q = (n_feat + 3) / 4;
#define GNNX_SDDMM(G, CPL) \
    return launch_sddmm<G, CPL>(vec, n_rows, n_feat, nnz, d_rowptr, d_colidx, d_L, ldl, d_R, ldr, d_rowscale, d_colscale, d_out, st)
    if (Q <= 1) GNNX_SDDMM(1, 1);
    if (Q <= 2) GNNX_SDDMM(2, 1);
    if (Q <= 4) GNNX_SDDMM(4, 1);
    if (Q <= 8) GNNX_SDDMM(8, 1);
    if (Q <= 16) GNNX_SDDMM(16, 1);
    if (Q <= 32) GNNX_SDDMM(32, 1);
    if (Q <= 64) GNNX_SDDMM(64, 1);
    if (Q <= 128) GNNX_SDDMM(64, 2);
    if (Q <= 192) GNNX_SDDMM(64, 3);
    if (Q <= 256) GNNX_SDDMM(64, 4);
#undef GNNX_SDDMM
    const int64_t blocks = ceil_div(ceil_div(nnz, kEntriesPerGroup) * 64, 256);
    if (vec)
        hipLaunchKernelGGL(sddmm_wide_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, st, n_rows, n_feat, nnz, d_rowptr, d_colidx, d_L, ldl,
                           d_R, ldr, d_rowscale, d_colscale, d_out);
    else
        hipLaunchKernelGGL(sddmm_wide_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, st, n_rows, n_feat, nnz, d_rowptr, d_colidx, d_L, ldl,
                           d_R, ldr, d_rowscale, d_colscale, d_out);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_csr_transpose_map(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                    const int32_t *d_rowptr_t, const int32_t *d_colidx_t, int32_t *d_map_t, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0 && nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(d_rowptr && d_rowptr_t, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(nnz == 0 || (d_colidx && d_colidx_t && d_map_t), GNNX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = as_stream(stream);
    int32_t ends[2] = {0, 0};
    GNNX_HIP_CHECK(hipMemcpyAsync(&ends[0], d_rowptr + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipMemcpyAsync(&ends[1], d_rowptr_t + n_cols, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(ends[0] == nnz && ends[1] == nnz, GNNX_ERR_INDEX_RANGE, "rowptr[n_rows] = %d, rowptr_t[n_cols] = %d, nnz = %lld disagree", ends[0],
                 ends[1], (long long)nnz);
    if (nnz == 0) return GNNX_OK;
    GNNX_REQUIRE(n_rows > 0 && n_cols > 0, GNNX_ERR_INDEX_RANGE, "entries in a matrix without rows or columns");
    int32_t *bad = nullptr;
    DeviceFreeSync guard;
    GNNX_HIP_CHECK(hipMalloc(&guard.p, sizeof(int32_t)));
    bad = static_cast<int32_t *>(guard.p);
    GNNX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    const uint32_t blocks = entry_blocks(nnz);
    hipLaunchKernelGGL(csr_ascending_kernel, dim3(blocks), dim3(256), 0, st, d_rowptr, d_colidx, n_rows, n_cols, nnz, bad);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_ascending_kernel, dim3(blocks), dim3(256), 0, st, d_rowptr_t, d_colidx_t, n_cols, n_rows, nnz, bad);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL(transpose_map_kernel, dim3(blocks), dim3(256), 0, st, d_rowptr, d_colidx, d_rowptr_t, d_colidx_t, n_rows, n_cols, nnz,
                       d_map_t, bad);
    GNNX_LAUNCH_CHECK();
    int32_t h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!(h_bad & 1), GNNX_ERR_INDEX_RANGE, "a row's columns are not strictly ascending inside [0, n_cols)");
    GNNX_REQUIRE(!(h_bad & 2), GNNX_ERR_INDEX_RANGE, "an entry of the transposed pattern has no partner");
    return GNNX_OK;
}
