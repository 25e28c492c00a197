// Query inference: the receptive field of a vertex set, layer by layer (reference graph.cpp:170-191 is the layer, :68-75 why a vertex
// is not its own neighbour, :130-151 the masks whose evaluation this serves).  For an ascending row list R of a CSR:
//   frontier marking   mark[c] = 1 for every column c stored in the rows R (byte stores; many lanes storing the same 1 is the only race)
//   position table     pos[R[k]] = k, -1 everywhere else
//   row extraction     the CSR of the k listed rows: rowptr' = exclusive scan of their lengths, entries copied in STORED ORDER (the
//                      summation order of the aggregation, also on a relabelled graph) with columns renumbered through a position table
//   renumbering        colidx[q] = pos[colidx[q]] in place, for a block that was made with original column ids (gnnx_csr_sample_rows)
// Marking and extraction work in the NON-ZERO domain of the LISTED rows, as restrict_* of gnnx_masked.hip does over the whole graph:
// the listed lengths are scanned, the listed entries cut into chunks of 64, one wavefront a chunk; the owning listed row is found by
// search in the scanned offsets (two wave-uniform searches bracket the chunk, one short search per lane inside the bracket).  A hub row
// of 250 000 entries is 3 907 chunks spread over the device; a list of 10^6 one-entry rows is 15 625 chunks.  Cost O(k + entries of
// the listed rows); nothing reads the whole graph.
// Integer work only: no floating-point arithmetic, no atomics but the error flag; every output has the same bits run to run.
#include "gnnx_common.h"

#include <rocprim/device/device_scan.hpp>

using namespace gnnx;

namespace {

constexpr int32_t kBadColumn = 1, kBadRowList = 2;

// len[k] = entries of row rows[k] (0 for a row the list should not hold); len[n_listed] = 0 (its scanned value is the total).
// The list must be ascending without repeats inside [0, n_rows): anything else raises kBadRowList and contributes no entries.
__global__ __launch_bounds__(256) void listed_len_kernel(const int32_t *rowptr, int32_t n_rows, const int32_t *rows, int64_t n_listed,
                                                          int64_t *len, int32_t *bad)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > n_listed) return;
    int64_t l = 0;
    if (k < n_listed) {
        const int32_t r = rows[k];
        if (r < 0 || r >= n_rows || (k > 0 && rows[k - 1] >= r)) {
            atomicOr(bad, kBadRowList);
        } else {
            l = (int64_t)rowptr[r + 1] - (int64_t)rowptr[r];
            if (l < 0) l = 0;   // (a rowptr that gnnx_csr_validate would refuse: stay inside the arrays)
        }
    }
    len[k] = l;
}

// largest k in [lo, hi] with off[k] <= p (off[lo] <= p is given).  Empty listed rows share their offset with the row behind them:
// the largest such k is the row that owns entry p.
__device__ __forceinline__ int64_t listed_row_of(const int64_t *off, int64_t lo, int64_t hi, int64_t p)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One wavefront per chunk of 64 consecutive entries of the listed rows.  kExtract = false: mark the columns.  kExtract = true: copy
// the entries to position p of the compact CSR, columns through `pos` when given.
template <bool kExtract>
__global__ __launch_bounds__(256) void listed_entries_kernel(const int32_t *rowptr, const int32_t *colidx, const float *vals, int32_t n_cols,
                                                              const int32_t *rows, int64_t n_listed, const int64_t *off, int64_t total,
                                                              uint8_t *mark, const int32_t *pos, int32_t *colidx_out, float *vals_out,
                                                              int32_t *bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t p0 = w * 64, p = p0 + lane;
    if (p0 >= total) return;   // wave-uniform
    const int64_t plast = p0 + 63 < total ? p0 + 63 : total - 1;
    const int64_t k0 = listed_row_of(off, 0, n_listed - 1, p0);
    const int64_t k1 = listed_row_of(off, k0, n_listed - 1, plast);
    if (p >= total) return;
    const int64_t k = listed_row_of(off, k0, k1, p);
    const int64_t src = (int64_t)rowptr[rows[k]] + (p - off[k]);
    const int32_t c = colidx[src];
    const bool in_range = c >= 0 && c < n_cols;
    if (!in_range) atomicOr(bad, kBadColumn);   // refused, never read or written behind an array
    if (kExtract) {
        int32_t q = c;
        if (pos) {
            q = in_range ? pos[c] : -1;
            if (in_range && q < 0) atomicOr(bad, kBadColumn);   // a column that is not in the set
        }
        colidx_out[p] = q;
        if (vals_out) vals_out[p] = vals[src];
    } else if (in_range) {
        mark[c] = 1;
    }
}

__global__ __launch_bounds__(256) void offsets_to_rowptr_kernel(const int64_t *off, int64_t n_listed, int32_t *rowptr_out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k <= n_listed) rowptr_out[k] = (int32_t)off[k];
}

__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t *v, int64_t n, int32_t value)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = value;
}

__global__ __launch_bounds__(256) void positions_kernel(const int32_t *rows, int64_t n_listed, int64_t n, int32_t *pos, int32_t *bad)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_listed) return;
    const int32_t r = rows[k];
    if (r < 0 || r >= n || (k > 0 && rows[k - 1] >= r)) atomicOr(bad, kBadRowList);
    else pos[r] = (int32_t)k;
}

// colidx[q] = pos[colidx[q]] in place; an entry without a position (a column outside the table, or one that maps to -1) becomes -1
__global__ __launch_bounds__(256) void renumber_cols_kernel(int64_t nnz, int32_t *colidx, const int32_t *pos, int64_t n_cols, int32_t *bad)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nnz) return;
    const int32_t c = colidx[q];
    const int32_t p = c >= 0 && c < n_cols ? pos[c] : -1;
    if (p < 0) atomicOr(bad, kBadColumn);
    colidx[q] = p < 0 ? -1 : p;
}

struct ListedWs {
    int64_t *len, *off;
    int32_t *bad;
    void *prim;
    size_t prim_bytes, total;
};

hipError_t listed_ws(int64_t n_listed, char *base, ListedWs &w)
{
    size_t scan_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan_bytes, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n_listed + 1,
                                           rocprim::plus<int64_t>());
    if (e != hipSuccess) return e;
    Carver c(base);
    w.len = c.take<int64_t>((size_t)n_listed + 1, 256);
    w.off = c.take<int64_t>((size_t)n_listed + 1, 256);
    w.bad = c.take<int32_t>(64, 256);
    w.prim = c.take<char>(scan_bytes, 256);
    w.prim_bytes = scan_bytes;
    w.total = c.bytes() + 256;   // room to align the caller's pointer
    return hipSuccess;
}

// lengths of the listed rows -> scanned offsets in w.off; *total_out (host) = entries of the listed rows.  Synchronises.
int listed_offsets(const int32_t *d_rowptr, int32_t n_rows, const int32_t *d_rows, int64_t n_listed, const ListedWs &w, hipStream_t st,
                   int64_t *total_out)
{
    GNNX_HIP_CHECK(hipMemsetAsync(w.bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(listed_len_kernel, dim3((uint32_t)ceil_div(n_listed + 1, 256)), dim3(256), 0, st, d_rowptr, n_rows, d_rows, n_listed, w.len,
                       w.bad);
    GNNX_LAUNCH_CHECK();
    size_t prim_bytes = w.prim_bytes;
    GNNX_HIP_CHECK(rocprim::exclusive_scan(w.prim, prim_bytes, w.len, w.off, (int64_t)0, (size_t)n_listed + 1, rocprim::plus<int64_t>(), st));
    int64_t total = 0;
    int32_t h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&total, w.off + n_listed, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, w.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "listed rows must be ascending, without repeats, inside [0, n_rows)");
    GNNX_REQUIRE(total < (1ll << 31), GNNX_ERR_UNSUPPORTED, "the listed rows hold %lld entries: must be < 2^31 (int32 CSR offsets)",
                 (long long)total);
    *total_out = total;
    return GNNX_OK;
}

int read_bad(const ListedWs &w, hipStream_t st, int32_t *h_bad)
{
    GNNX_HIP_CHECK(hipMemcpyAsync(h_bad, w.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    return GNNX_OK;
}

inline uint32_t entry_groups(int64_t total) { return (uint32_t)ceil_div(ceil_div(total, 64), 4); }

}  // namespace

GNNX_API int gnnx_frontier_mark_workspace(int64_t n_listed, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_listed >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    ListedWs w;
    GNNX_HIP_CHECK(listed_ws(n_listed, nullptr, w));
    *bytes = w.total;
    return GNNX_OK;
}

GNNX_API int gnnx_frontier_mark(const int32_t *d_rowptr, const int32_t *d_colidx, int32_t n_rows, int32_t n_cols, const int32_t *d_rows,
                                int64_t n_listed, uint8_t *d_mark, int64_t *nnz_listed_out, void *d_workspace, size_t workspace_bytes,
                                void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_listed >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz_listed_out, GNNX_ERR_INVALID_ARG, "null count pointer");
    *nnz_listed_out = 0;
    if (n_listed == 0) return GNNX_OK;   // no rows: nothing to mark
    GNNX_REQUIRE(n_listed <= n_rows, GNNX_ERR_INVALID_ARG, "more listed rows (%lld) than rows (%d)", (long long)n_listed, n_rows);
    GNNX_REQUIRE(d_rowptr && d_rows, GNNX_ERR_INVALID_ARG, "null pointer");
    ListedWs w;
    GNNX_HIP_CHECK(listed_ws(n_listed, d_workspace ? aligned_base(d_workspace) : nullptr, w));
    GNNX_REQUIRE(d_workspace && workspace_bytes >= w.total, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    hipStream_t st = as_stream(stream);
    int64_t total = 0;
    if (int rc = listed_offsets(d_rowptr, n_rows, d_rows, n_listed, w, st, &total)) return rc;
    *nnz_listed_out = total;
    if (total == 0) return GNNX_OK;
    GNNX_REQUIRE(d_colidx && d_mark, GNNX_ERR_INVALID_ARG, "null pointer");
    hipLaunchKernelGGL(listed_entries_kernel<false>, dim3(entry_groups(total)), dim3(256), 0, st, d_rowptr, d_colidx, (const float *)nullptr,
                       n_cols, d_rows, n_listed, w.off, total, d_mark, (const int32_t *)nullptr, (int32_t *)nullptr, (float *)nullptr, w.bad);
    GNNX_LAUNCH_CHECK();
    int32_t h_bad = 0;
    if (int rc = read_bad(w, st, &h_bad)) return rc;
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "column id outside [0, n_cols)");
    return GNNX_OK;
}

GNNX_API int gnnx_rows_to_positions_workspace(size_t *bytes)
{
    GNNX_REQUIRE(bytes, GNNX_ERR_INVALID_ARG, "null pointer");
    *bytes = 512;
    return GNNX_OK;
}

GNNX_API int gnnx_rows_to_positions(const int32_t *d_rows, int64_t n_listed, int64_t n, int32_t *d_pos, void *d_workspace,
                                    size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_listed >= 0 && n >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n < (1ll << 31), GNNX_ERR_UNSUPPORTED, "n must be < 2^31 (int32 row ids)");
    GNNX_REQUIRE(n_listed <= n, GNNX_ERR_INVALID_ARG, "more listed rows (%lld) than rows (%lld)", (long long)n_listed, (long long)n);
    if (n == 0) return GNNX_OK;
    GNNX_REQUIRE(d_pos && (d_rows || n_listed == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(d_workspace && workspace_bytes >= 512, GNNX_ERR_WORKSPACE, "workspace %zu < required 512", workspace_bytes);
    hipStream_t st = as_stream(stream);
    int32_t *bad = reinterpret_cast<int32_t *>(aligned_base(d_workspace));
    GNNX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(fill_i32_kernel, dim3((uint32_t)ceil_div(n, 256)), dim3(256), 0, st, d_pos, n, (int32_t)-1);
    GNNX_LAUNCH_CHECK();
    if (n_listed) {
        hipLaunchKernelGGL(positions_kernel, dim3((uint32_t)ceil_div(n_listed, 256)), dim3(256), 0, st, d_rows, n_listed, n, d_pos, bad);
        GNNX_LAUNCH_CHECK();
    }
    int32_t h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "listed rows must be ascending, without repeats, inside [0, n)");
    return GNNX_OK;
}

GNNX_API int gnnx_csr_extract_rows_workspace(int64_t n_listed, size_t *bytes)
{
    return gnnx_frontier_mark_workspace(n_listed, bytes);
}

GNNX_API int gnnx_csr_extract_rows(int32_t n_rows, int32_t n_cols, const int32_t *d_rowptr, const int32_t *d_colidx, const float *d_vals,
                                   const int32_t *d_rows, int64_t n_listed, const int32_t *d_col_pos, int32_t *d_rowptr_out,
                                   int32_t *d_colidx_out, float *d_vals_out, int64_t nnz_capacity, int64_t *nnz_out, void *d_workspace,
                                   size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_listed >= 0 && nnz_capacity >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz_out, GNNX_ERR_INVALID_ARG, "null count pointer");
    *nnz_out = 0;
    GNNX_REQUIRE(n_listed <= n_rows, GNNX_ERR_INVALID_ARG, "more listed rows (%lld) than rows (%d)", (long long)n_listed, n_rows);
    GNNX_REQUIRE(!d_vals == !d_vals_out, GNNX_ERR_INVALID_ARG, "vals and vals_out go together");
    GNNX_REQUIRE(d_rowptr_out, GNNX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = as_stream(stream);
    if (n_listed == 0) {   // a CSR of no rows: rowptr' = [0]
        GNNX_HIP_CHECK(hipMemsetAsync(d_rowptr_out, 0, sizeof(int32_t), st));
        GNNX_HIP_CHECK(hipStreamSynchronize(st));
        return GNNX_OK;
    }
    GNNX_REQUIRE(d_rowptr && d_rows, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(d_rowptr_out != d_rowptr, GNNX_ERR_INVALID_ARG, "in place is not supported");
    ListedWs w;
    GNNX_HIP_CHECK(listed_ws(n_listed, d_workspace ? aligned_base(d_workspace) : nullptr, w));
    GNNX_REQUIRE(d_workspace && workspace_bytes >= w.total, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    int64_t total = 0;
    if (int rc = listed_offsets(d_rowptr, n_rows, d_rows, n_listed, w, st, &total)) return rc;
    *nnz_out = total;   // also when the capacity is refused: what the caller has to offer
    GNNX_REQUIRE(total <= nnz_capacity, GNNX_ERR_INVALID_ARG, "the listed rows hold %lld entries, nnz_capacity is %lld (nothing was written)",
                 (long long)total, (long long)nnz_capacity);
    hipLaunchKernelGGL(offsets_to_rowptr_kernel, dim3((uint32_t)ceil_div(n_listed + 1, 256)), dim3(256), 0, st, w.off, n_listed, d_rowptr_out);
    GNNX_LAUNCH_CHECK();
    if (total) {
        GNNX_REQUIRE(d_colidx && d_colidx_out && d_colidx_out != d_colidx, GNNX_ERR_INVALID_ARG, "null pointer, or in place");
        hipLaunchKernelGGL(listed_entries_kernel<true>, dim3(entry_groups(total)), dim3(256), 0, st, d_rowptr, d_colidx, d_vals, n_cols, d_rows,
                           n_listed, w.off, total, (uint8_t *)nullptr, d_col_pos, d_colidx_out, d_vals_out, w.bad);
        GNNX_LAUNCH_CHECK();
    }
    int32_t h_bad = 0;
    if (int rc = read_bad(w, st, &h_bad)) return rc;
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE,
                 d_col_pos ? "a column of the listed rows is outside [0, n_cols) or not in the position table's set" : "column id outside [0, n_cols)");
    return GNNX_OK;
}

GNNX_API int gnnx_csr_renumber_cols(int64_t nnz, int32_t *d_colidx, const int32_t *d_pos, int64_t n_cols, void *d_workspace, size_t workspace_bytes,
                                    void *stream)
{
    GNNX_REQUIRE(nnz >= 0 && n_cols >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31) && n_cols < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz and n_cols must be < 2^31 (int32 CSR)");
    if (nnz == 0) return GNNX_OK;
    GNNX_REQUIRE(d_colidx && (d_pos || n_cols == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(d_workspace && workspace_bytes >= 256, GNNX_ERR_WORKSPACE, "workspace %zu < required 256", workspace_bytes);
    hipStream_t st = as_stream(stream);
    int32_t *bad = reinterpret_cast<int32_t *>((reinterpret_cast<uintptr_t>(d_workspace) + 3u) & ~(uintptr_t)3u);
    GNNX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(renumber_cols_kernel, dim3((uint32_t)ceil_div(nnz, 256)), dim3(256), 0, st, nnz, d_colidx, d_pos, n_cols, bad);
    GNNX_LAUNCH_CHECK();
    int32_t h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "a column is outside [0, n_cols) or has no position in the table (such entries are now -1)");
    return GNNX_OK;
}
