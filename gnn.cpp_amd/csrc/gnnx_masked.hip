// Semi-supervised training: a label mask as a row list, a CSR restricted to the entries a mask keeps, per-row argmax and accuracy
// (reference graph.h: Data::set_mask with train / val / test masks; functional.h:59-61 argmax).  The loss over a row list is
// gnnx_train.hip's.
//   mask -> rows      wave-wide ballot compaction: 64 mask bytes per wavefront, counts scanned, lanes write at popcount positions
//   CSR restriction   works in the NON-ZERO domain, not per row: the entry array is cut into chunks of 64 consecutive entries, one
//                     wavefront a chunk (coalesced reads of colidx / vals), keep bits by __ballot, positions from a scan over the
//                     chunk counts + popcount of the lanes below.  Entries of one row are consecutive in the array, so surviving
//                     entries keep their stored order inside the row, and a hub row of 10^6 entries is simply 15 625 chunks spread
//                     over the device.  rowptr' comes from the same scan: survivors in front of rowptr[r].
//   argmax            one wavefront per row, (max, lowest index) butterfly
// No floating-point atomics: every float result has the same bits run to run (integer counters only).
#include "gnnx_common.h"

#include <rocprim/device/device_scan.hpp>

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// ---------------------------------------------------------------------------------------------------- mask -> rows
// cnt[w] = set bytes among mask[64 w .. 64 w + 63]; cnt[n_chunks] = 0 (its scanned value is the total)
__global__ __launch_bounds__(256) void mask_count_kernel(const uint8_t *mask, int64_t n, int64_t n_chunks, int32_t *cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w > n_chunks) return;
    const int64_t i = w * 64 + lane;
    const bool keep = w < n_chunks && i < n && mask[i] != 0;
    const uint64_t b = __ballot(keep);
    if (lane == 0) cnt[w] = __popcll(b);
}

__global__ __launch_bounds__(256) void mask_fill_kernel(const uint8_t *mask, int64_t n, int64_t n_chunks, const int32_t *pos, int32_t *rows)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_chunks) return;
    const int64_t i = w * 64 + lane;
    const bool keep = i < n && mask[i] != 0;
    const uint64_t b = __ballot(keep);
    if (keep) rows[pos[w] + __popcll(b & lanes_below(lane))] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------------- CSR restriction
// largest r in [lo, hi] with rowptr[r] <= p (rowptr[lo] <= p is given)
__device__ __forceinline__ int32_t row_of(const int32_t *rowptr, int32_t lo, int32_t hi, int64_t p)
{
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if ((int64_t)rowptr[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One wavefront per chunk of 64 consecutive entries: keep bits -> bits[chunk], their count -> cnt[chunk]; cnt[n_chunks] = 0.
// The row of an entry is only looked up when there is a row mask: the chunk's first and last entry bracket the rows of the other 62
// (two wave-uniform searches over all rows, then a search over the few rows in between per lane).
__global__ __launch_bounds__(256) void restrict_flag_kernel(const int32_t *rowptr, const int32_t *colidx, int32_t n_rows, int32_t n_cols,
                                                             int64_t nnz, int64_t n_chunks, const uint8_t *row_keep, const uint8_t *col_keep,
                                                             uint64_t *bits, int32_t *cnt, int32_t *bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w > n_chunks) return;
    if (w == n_chunks) {
        if (lane == 0) cnt[w] = 0;
        return;
    }
    const int64_t p0 = w * 64, p = p0 + lane;
    bool keep = p < nnz;
    if (row_keep) {   // wave-uniform
        const int64_t plast = p0 + 63 < nnz ? p0 + 63 : nnz - 1;
        const int32_t r0 = row_of(rowptr, 0, n_rows - 1, p0);
        const int32_t r1 = row_of(rowptr, r0, n_rows - 1, plast);
        if (keep) keep = row_keep[row_of(rowptr, r0, r1, p)] != 0;
    }
    if (keep && col_keep) {
        const int32_t c = colidx[p];
        if (c < 0 || c >= n_cols) {   // a column id outside the mask: refused, never read behind the array
            atomicOr(bad, 1);
            keep = false;
        } else {
            keep = col_keep[c] != 0;
        }
    }
    const uint64_t b = __ballot(keep);
    if (lane == 0) {
        bits[w] = b;
        cnt[w] = __popcll(b);
    }
}

__global__ __launch_bounds__(256) void restrict_fill_kernel(const int32_t *colidx, const float *vals, int64_t nnz, int64_t n_chunks,
                                                             const uint64_t *bits, const int32_t *pos, int32_t *colidx_out, float *vals_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_chunks) return;
    const uint64_t b = bits[w];
    if (b == 0) return;   // wave-uniform
    const int64_t p = w * 64 + lane;
    if ((b >> lane) & 1ull) {
        const int64_t q = (int64_t)pos[w] + __popcll(b & lanes_below(lane));
        colidx_out[q] = colidx[p];
        if (vals_out) vals_out[q] = vals[p];
    }
}

// rowptr'[r] = survivors in front of entry rowptr[r]
__global__ __launch_bounds__(256) void restrict_rowptr_kernel(const int32_t *rowptr, int32_t n_rows, int64_t nnz, int64_t n_chunks,
                                                               const uint64_t *bits, const int32_t *pos, int32_t *rowptr_out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_rows) return;
    int64_t p = rowptr[r];
    if (p < 0) p = 0;   // (a rowptr that gnnx_csr_validate would refuse: stay inside the arrays)
    if (p >= nnz) {
        rowptr_out[r] = pos[n_chunks];
        return;
    }
    const int64_t c = p >> 6;
    rowptr_out[r] = pos[c] + __popcll(bits[c] & lanes_below((int)(p & 63)));
}

struct RestrictWs {
    int32_t *cnt, *pos, *bad;
    uint64_t *bits;
    void *prim;
    size_t prim_bytes, total;
};

hipError_t restrict_ws(int64_t n_chunks, char *base, RestrictWs &w)
{
    size_t scan_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan_bytes, (int32_t *)nullptr, (int32_t *)nullptr, 0, (size_t)n_chunks + 1,
                                           rocprim::plus<int32_t>());
    if (e != hipSuccess) return e;
    Carver c(base);
    w.cnt = c.take<int32_t>((size_t)n_chunks + 1, 256);
    w.pos = c.take<int32_t>((size_t)n_chunks + 1, 256);
    w.bits = c.take<uint64_t>((size_t)n_chunks + 1, 256);
    w.bad = c.take<int32_t>(64, 256);
    w.prim = c.take<char>(scan_bytes, 256);
    w.prim_bytes = scan_bytes;
    w.total = c.bytes() + 256;   // room to align the caller's pointer
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------- argmax / accuracy
// One wavefront per listed row (rows == NULL: row i): lanes stride the classes keeping (max, first index), then a butterfly that
// prefers the larger value and, among equal values, the lower index.  pred[i] (when given) = the class; *correct += pred == target.
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float *X, int64_t ldx, const int32_t *target, const int32_t *rows,
                                                           int64_t n_listed, int64_t n_rows, int32_t n_cls, int32_t *pred,
                                                           unsigned long long *correct, int32_t *bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    unsigned long long hits = 0;
    for (int64_t i = wave; i < n_listed; i += n_waves) {
        const int64_t row = rows ? (int64_t)rows[i] : i;
        if (row < 0 || row >= n_rows) {   // wave-uniform
            if (lane == 0) atomicOr(bad, 2);
            continue;
        }
        const float *x = X + row * ldx;
        float bv = -INFINITY;
        int32_t bi = INT32_MAX;
        for (int32_t c = lane; c < n_cls; c += 64) {
            const float v = x[c];
            if (bi == INT32_MAX || v > bv) {
                bv = v;
                bi = c;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int32_t oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            if (pred) pred[i] = bi;
            if (target && target[row] == bi) hits++;
        }
    }
    if (lane == 0 && correct && hits) atomicAdd(correct, hits);
}

int argmax_impl(const float *d_logits, int64_t ldx, const int32_t *d_target, const int32_t *d_rows, int64_t n_listed, int64_t n_rows,
                int32_t n_classes, int32_t *d_pred, int64_t *correct_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_listed >= 0 && n_rows >= 0 && n_classes > 0, GNNX_ERR_INVALID_ARG, "negative size or no classes");
    GNNX_REQUIRE(d_rows || n_listed == n_rows, GNNX_ERR_INVALID_ARG, "no row list: n_listed must be n_rows");
    if (correct_out) *correct_out = 0;
    if (n_listed == 0) return GNNX_OK;
    GNNX_REQUIRE(d_logits && ldx >= n_classes, GNNX_ERR_INVALID_ARG, "null pointer or ld < n_classes");
    GNNX_REQUIRE(d_workspace && workspace_bytes >= 512, GNNX_ERR_WORKSPACE, "workspace %zu < required 512", workspace_bytes);
    hipStream_t st = as_stream(stream);
    char *base = aligned_base(d_workspace);
    unsigned long long *correct = reinterpret_cast<unsigned long long *>(base);
    int32_t *bad = reinterpret_cast<int32_t *>(base + 8);
    GNNX_HIP_CHECK(hipMemsetAsync(base, 0, 16, st));
    int64_t groups = ceil_div(n_listed, 4);
    if (groups > 4096) groups = 4096;
    hipLaunchKernelGGL(argmax_rows_kernel, dim3((uint32_t)groups), dim3(256), 0, st, d_logits, ldx, d_target, d_rows, n_listed, n_rows, n_classes,
                       d_pred, correct_out ? correct : nullptr, bad);
    GNNX_LAUNCH_CHECK();
    struct { unsigned long long correct; int32_t bad, pad; } h = {0, 0, 0};
    GNNX_HIP_CHECK(hipMemcpyAsync(&h, base, 16, hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!h.bad, GNNX_ERR_INDEX_RANGE, "listed row outside [0, n_rows)");
    if (correct_out) *correct_out = (int64_t)h.correct;
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_mask_to_rows_workspace(int64_t n, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    RestrictWs w;
    GNNX_HIP_CHECK(restrict_ws(ceil_div(n, 64), nullptr, w));
    *bytes = w.total;
    return GNNX_OK;
}

GNNX_API int gnnx_mask_to_rows(const uint8_t *d_mask, int64_t n, int32_t *d_rows, int32_t *n_rows_out, void *d_workspace,
                               size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n >= 0 && n_rows_out, GNNX_ERR_INVALID_ARG, "negative size or null count pointer");
    GNNX_REQUIRE(n < (1ll << 31), GNNX_ERR_UNSUPPORTED, "n must be < 2^31 (int32 row ids)");
    *n_rows_out = 0;
    if (n == 0) return GNNX_OK;
    GNNX_REQUIRE(d_mask && d_rows, GNNX_ERR_INVALID_ARG, "null pointer");
    const int64_t n_chunks = ceil_div(n, 64);
    RestrictWs w;
    GNNX_HIP_CHECK(restrict_ws(n_chunks, d_workspace ? aligned_base(d_workspace) : nullptr, w));
    GNNX_REQUIRE(d_workspace && workspace_bytes >= w.total, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    hipStream_t st = as_stream(stream);
    const uint32_t groups = (uint32_t)ceil_div(n_chunks + 1, 4);
    hipLaunchKernelGGL(mask_count_kernel, dim3(groups), dim3(256), 0, st, d_mask, n, n_chunks, w.cnt);
    GNNX_LAUNCH_CHECK();
    GNNX_HIP_CHECK(rocprim::exclusive_scan(w.prim, w.prim_bytes, w.cnt, w.pos, 0, (size_t)n_chunks + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(mask_fill_kernel, dim3(groups), dim3(256), 0, st, d_mask, n, n_chunks, w.pos, d_rows);
    GNNX_LAUNCH_CHECK();
    int32_t total = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&total, w.pos + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    *n_rows_out = total;
    return GNNX_OK;
}

GNNX_API int gnnx_csr_restrict_workspace(int32_t n_rows, int64_t nnz, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_rows >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    RestrictWs w;
    GNNX_HIP_CHECK(restrict_ws(ceil_div(nnz, 64), nullptr, w));
    *bytes = w.total;
    return GNNX_OK;
}

GNNX_API int gnnx_csr_restrict(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                               const float *d_vals, const uint8_t *d_row_keep, const uint8_t *d_col_keep, int32_t *d_rowptr_out,
                               int32_t *d_colidx_out, float *d_vals_out, int64_t *nnz_out, void *d_workspace, size_t workspace_bytes,
                               void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_UNSUPPORTED, "nnz must be < 2^31 (int32 CSR offsets)");
    GNNX_REQUIRE(d_rowptr && d_rowptr_out && nnz_out, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(!d_vals == !d_vals_out, GNNX_ERR_INVALID_ARG, "vals and vals_out go together");
    GNNX_REQUIRE(d_rowptr_out != d_rowptr && (nnz == 0 || d_colidx_out != d_colidx), GNNX_ERR_INVALID_ARG, "in place is not supported");
    hipStream_t st = as_stream(stream);
    *nnz_out = 0;
    int32_t h_end = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_end, d_rowptr + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE((int64_t)h_end == nnz, GNNX_ERR_INVALID_ARG, "nnz = %lld, but rowptr[n_rows] = %d", (long long)nnz, h_end);
    if (nnz == 0) {
        GNNX_HIP_CHECK(hipMemsetAsync(d_rowptr_out, 0, sizeof(int32_t) * ((size_t)n_rows + 1), st));
        GNNX_HIP_CHECK(hipStreamSynchronize(st));
        return GNNX_OK;
    }
    GNNX_REQUIRE(d_colidx && d_colidx_out, GNNX_ERR_INVALID_ARG, "null pointer");
    const int64_t n_chunks = ceil_div(nnz, 64);
    RestrictWs w;
    GNNX_HIP_CHECK(restrict_ws(n_chunks, d_workspace ? aligned_base(d_workspace) : nullptr, w));
    GNNX_REQUIRE(d_workspace && workspace_bytes >= w.total, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    GNNX_HIP_CHECK(hipMemsetAsync(w.bad, 0, sizeof(int32_t), st));
    const uint32_t groups = (uint32_t)ceil_div(n_chunks + 1, 4);
    hipLaunchKernelGGL(restrict_flag_kernel, dim3(groups), dim3(256), 0, st, d_rowptr, d_colidx, n_rows, n_cols, nnz, n_chunks, d_row_keep,
                       d_col_keep, w.bits, w.cnt, w.bad);
    GNNX_LAUNCH_CHECK();
    GNNX_HIP_CHECK(rocprim::exclusive_scan(w.prim, w.prim_bytes, w.cnt, w.pos, 0, (size_t)n_chunks + 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(restrict_fill_kernel, dim3(groups), dim3(256), 0, st, d_colidx, d_vals, nnz, n_chunks, w.bits, w.pos, d_colidx_out,
                       d_vals_out);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL(restrict_rowptr_kernel, dim3((uint32_t)ceil_div((int64_t)n_rows + 1, 256)), dim3(256), 0, st, d_rowptr, n_rows, nnz,
                       n_chunks, w.bits, w.pos, d_rowptr_out);
    GNNX_LAUNCH_CHECK();
    int32_t total = 0, h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&total, w.pos + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, w.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "column id outside [0, n_cols)");
    *nnz_out = total;
    return GNNX_OK;
}

GNNX_API int gnnx_argmax_rows_workspace(size_t *bytes)
{
    GNNX_REQUIRE(bytes, GNNX_ERR_INVALID_ARG, "null pointer");
    *bytes = 512;
    return GNNX_OK;
}

GNNX_API int gnnx_argmax_rows_f32(const float *d_logits, int64_t ldx, int64_t n_rows, int32_t n_classes, int32_t *d_pred, void *d_workspace,
                                  size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(d_pred || n_rows == 0, GNNX_ERR_INVALID_ARG, "null pointer");
    return argmax_impl(d_logits, ldx, nullptr, nullptr, n_rows, n_rows, n_classes, d_pred, nullptr, d_workspace, workspace_bytes, stream);
}

GNNX_API int gnnx_accuracy_rows_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, const int32_t *d_rows, int64_t n_listed,
                                    int64_t n_rows, int32_t n_classes, int32_t *d_pred, int64_t *correct_out, void *d_workspace,
                                    size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(correct_out && (d_target || n_listed == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    return argmax_impl(d_logits, ldx, d_target, d_rows, n_listed, n_rows, n_classes, d_pred, correct_out, d_workspace, workspace_bytes, stream);
}
