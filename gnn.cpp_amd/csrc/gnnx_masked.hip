// Semi-supervised training: a label mask as a row list, a CSR restricted to the entries a mask keeps, softmax cross-entropy over a
// row list, per-row argmax and accuracy (reference graph.h: Data::set_mask with train / val / test masks; functional.h:59-61 argmax).
//   mask -> rows      wave-wide ballot compaction: 64 mask bytes per wavefront, counts scanned, lanes write at popcount positions
//   CSR restriction   works in the NON-ZERO domain, not per row: the entry array is cut into chunks of 64 consecutive entries, one
//                     wavefront a chunk (coalesced reads of colidx / vals), keep bits by __ballot, positions from a scan over the
//                     chunk counts + popcount of the lanes below.  Entries of one row are consecutive in the array, so surviving
//                     entries keep their stored order inside the row, and a hub row of 10^6 entries is simply 15 625 chunks spread
//                     over the device.  rowptr' comes from the same scan: survivors in front of rowptr[r].
//   loss over rows    softmax_ce_kernel / softmax_ce_vec_kernel of gnnx_train.hip behind a row list: the same expression per element
//                     and the same order of the row sum, so listing every row gives the bits of gnnx_softmax_ce_f32's dlogits
//   argmax            one wavefront per row, (max, lowest index) butterfly
// No floating-point atomics: every float result has the same bits run to run (integer counters only).
#include "gnnx_common.h"

#include <rocprim/device/device_scan.hpp>

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

inline size_t align256(size_t v) { return (v + 255u) & ~(size_t)255u; }

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
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    w.cnt = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)n_chunks + 1)));
    w.pos = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)n_chunks + 1)));
    w.bits = reinterpret_cast<uint64_t *>(take(sizeof(uint64_t) * ((size_t)n_chunks + 1)));
    w.bad = reinterpret_cast<int32_t *>(take(256));
    w.prim = take(scan_bytes);
    w.prim_bytes = scan_bytes;
    w.total = off + 256;   // room to align the caller's pointer
    return hipSuccess;
}

inline char *aligned_base(void *p) { return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(p) + 255u) & ~(uintptr_t)255u); }

// ---------------------------------------------------------------------------------------------------- loss over a row list
// softmax_ce_kernel (gnnx_train.hip) behind a row list: wavefront i works on row rows[i]; per-row loss to row_loss[i]
__global__ __launch_bounds__(256) void ce_rows_kernel(const float *X, int64_t ldx, const int32_t *target, const int32_t *rows, int64_t n_listed,
                                                       int64_t n_rows, int32_t n_cls, float inv_n, float *row_loss, float *dX, int64_t ldd,
                                                       int32_t *bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_listed) return;
    const int64_t row = rows[i];
    if (row < 0 || row >= n_rows) {
        if (lane == 0) atomicOr(bad, 2);
        return;
    }
    const float *x = X + row * ldx;
    float sum = 0.f;
    for (int32_t c = lane; c < n_cls; c += 64) sum += expf(x[c]);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const int32_t t = target[row];
    if (t < 0 || t >= n_cls) {
        if (lane == 0) atomicOr(bad, 1);
        return;
    }
    const float denom = sum + 1e-20f;
    if (lane == 0 && row_loss) row_loss[i] = -logf(expf(x[t]) / denom);
    if (dX) {
        float *d = dX + row * ldd;
        const float rden = 1.0f / denom;
        for (int32_t c = lane; c < n_cls; c += 64) d[c] = (expf(x[c]) * rden - (c == t ? 1.f : 0.f)) * inv_n;
    }
}

// softmax_ce_vec_kernel (gnnx_train.hip) behind a row list: class counts that are a multiple of 4 and at most 1024, 16-byte aligned
// rows; a lane holds classes 256 k + 4 lane .. + 3, exp evaluated once per element, two listed rows in flight per wavefront, the
// column sums of the gradient rows a wavefront wrote kept in registers and stored as row `wave id` of the partials.
template <int KV>
__global__ __launch_bounds__(256) void ce_rows_vec_kernel(const float *X, int64_t ldx, const int32_t *target, const int32_t *rows,
                                                           int64_t n_listed, int64_t n_rows, int32_t n_cls, float inv_n, float *row_loss,
                                                           float *dX, int64_t ldd, int32_t *bad, float *colsum_partial)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    float4 cs[KV];
#pragma unroll
    for (int k = 0; k < KV; k++) cs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i0 = wave; i0 < n_listed; i0 += 2 * n_waves) {
        float4 e[2][KV];
        int32_t t[2];
        int64_t row[2];
        bool have[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int64_t i = i0 + u * n_waves;
            have[u] = i < n_listed;
            row[u] = have[u] ? (int64_t)rows[i] : 0;
            if (have[u] && (row[u] < 0 || row[u] >= n_rows)) {   // wave-uniform
                if (lane == 0) atomicOr(bad, 2);
                have[u] = false;
            }
            t[u] = have[u] ? target[row[u]] : 0;
#pragma unroll
            for (int k = 0; k < KV; k++) {
                const int32_t c = 256 * k + 4 * lane;
                e[u][k] = (have[u] && c < n_cls) ? *reinterpret_cast<const float4 *>(X + row[u] * ldx + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (!have[u]) continue;   // wave-uniform
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < KV; k++) {
                if (256 * k + 4 * lane < n_cls) {
                    e[u][k].x = expf(e[u][k].x);
                    e[u][k].y = expf(e[u][k].y);
                    e[u][k].z = expf(e[u][k].z);
                    e[u][k].w = expf(e[u][k].w);
                    sum += e[u][k].x;
                    sum += e[u][k].y;
                    sum += e[u][k].z;
                    sum += e[u][k].w;
                }
            }
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            if (t[u] < 0 || t[u] >= n_cls) {
                if (lane == 0) atomicOr(bad, 1);
                continue;
            }
            const float denom = sum + 1e-20f;
            if (lane == 0 && row_loss) row_loss[i0 + u * n_waves] = -logf(expf(X[row[u] * ldx + t[u]]) / denom);
            if (dX) {
                const float rden = 1.0f / denom;
#pragma unroll
                for (int k = 0; k < KV; k++) {
                    const int32_t c = 256 * k + 4 * lane;
                    if (c < n_cls) {
                        float4 d;
                        d.x = (e[u][k].x * rden - (c + 0 == t[u] ? 1.f : 0.f)) * inv_n;
                        d.y = (e[u][k].y * rden - (c + 1 == t[u] ? 1.f : 0.f)) * inv_n;
                        d.z = (e[u][k].z * rden - (c + 2 == t[u] ? 1.f : 0.f)) * inv_n;
                        d.w = (e[u][k].w * rden - (c + 3 == t[u] ? 1.f : 0.f)) * inv_n;
                        *reinterpret_cast<float4 *>(dX + row[u] * ldd + c) = d;
                        cs[k].x += d.x;
                        cs[k].y += d.y;
                        cs[k].z += d.z;
                        cs[k].w += d.w;
                    }
                }
            }
        }
    }
    if (colsum_partial) {
#pragma unroll
        for (int k = 0; k < KV; k++) {
            const int32_t c = 256 * k + 4 * lane;
            if (c < n_cls) *reinterpret_cast<float4 *>(colsum_partial + wave * n_cls + c) = cs[k];
        }
    }
}

// generic class counts: column sums of the listed gradient rows, one thread per class over a block of the list (a second pass over
// O(listed rows))
__global__ __launch_bounds__(256) void ce_rows_colsum_generic(const float *dX, int64_t ldd, const int32_t *rows, int64_t n_listed, int64_t n_rows,
                                                               int32_t n_cls, float *partial, int64_t rows_per_block)
{
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_block, i1 = i0 + rows_per_block < n_listed ? i0 + rows_per_block : n_listed;
    const int32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cls) return;
    float acc = 0.f;
    for (int64_t i = i0; i < i1; i++) {
        const int64_t row = rows[i];
        if (row >= 0 && row < n_rows) acc += dX[row * ldd + c];
    }
    partial[(int64_t)blockIdx.y * n_cls + c] = acc;
}

// out[c] = sum over the partial rows, 4 interleaved parts per column combined in part order (fixed order: deterministic)
__global__ __launch_bounds__(256) void rows_colsum_reduce(const float *partial, int32_t n_part, int32_t n_cls, float *out)
{
    __shared__ float red[256];
    const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int32_t f = blockIdx.x * 64 + c;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (f < n_cls) {
        int32_t b = part;
        for (; b + 12 < n_part; b += 16) {
            a0 += partial[(int64_t)b * n_cls + f];
            a1 += partial[(int64_t)(b + 4) * n_cls + f];
            a2 += partial[(int64_t)(b + 8) * n_cls + f];
            a3 += partial[(int64_t)(b + 12) * n_cls + f];
        }
        for (; b < n_part; b += 4) a0 += partial[(int64_t)b * n_cls + f];
    }
    red[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (part == 0 && f < n_cls) out[f] = ((red[c] + red[64 + c]) + red[128 + c]) + red[192 + c];
}

// deterministic two-stage sum of the per-row losses
__global__ __launch_bounds__(256) void rows_sum_stage1(const float *v, int64_t n, float *partial)
{
    __shared__ float red[256];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += v[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void rows_sum_stage2(const float *partial, int n_blocks, float scale, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float acc = 0.f;
        for (int b = 0; b < n_blocks; b++) acc += partial[b];
        *out = acc * scale;
    }
}

constexpr int kSumBlocks = 256;
constexpr int kCeMaxGroups = 2048;   // as gnnx_train.hip: at most this many workgroups of 4 wavefronts
constexpr int kCeGenericParts = 256;

inline int ce_groups(int64_t n_listed)
{
    int64_t gsz = ceil_div(n_listed, 8);   // 4 wavefronts, 2 rows in flight each
    return (int)(gsz < 1 ? 1 : (gsz > kCeMaxGroups ? kCeMaxGroups : gsz));
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

GNNX_API int gnnx_softmax_ce_rows_workspace(int64_t n_listed, int32_t n_classes, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_listed >= 0 && n_classes >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    const size_t parts = (size_t)(4 * ce_groups(n_listed) > kCeGenericParts ? 4 * ce_groups(n_listed) : kCeGenericParts);
    *bytes = sizeof(float) * ((size_t)n_listed + kSumBlocks + 64 + parts * (size_t)n_classes) + 512;
    return GNNX_OK;
}

GNNX_API int gnnx_softmax_ce_rows_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, const int32_t *d_rows, int64_t n_listed,
                                      int64_t n_rows, int32_t n_classes, int64_t n_total, float *d_loss, float *d_dlogits, int64_t ldd,
                                      float *d_colsum, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_listed > 0 && n_classes > 0, GNNX_ERR_INVALID_ARG, "empty row list (the mean over no rows is undefined)");
    GNNX_REQUIRE(n_rows >= n_listed, GNNX_ERR_INVALID_ARG, "more listed rows than rows");
    GNNX_REQUIRE(n_total >= n_listed, GNNX_ERR_INVALID_ARG, "n_total < n_listed");
    GNNX_REQUIRE(d_logits && d_target && d_rows && ldx >= n_classes, GNNX_ERR_INVALID_ARG, "null pointer or ld < n_classes");
    GNNX_REQUIRE(!d_dlogits || ldd >= n_classes, GNNX_ERR_INVALID_ARG, "ldd < n_classes");
    GNNX_REQUIRE(!d_colsum || d_dlogits, GNNX_ERR_INVALID_ARG, "column sums are those of dlogits: dlogits is null");
    size_t need = 0;
    gnnx_softmax_ce_rows_workspace(n_listed, n_classes, &need);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float *row_loss = reinterpret_cast<float *>(aligned_base(d_workspace));
    float *partial = row_loss + n_listed;
    int32_t *bad = reinterpret_cast<int32_t *>(partial + kSumBlocks);
    float *cpart = reinterpret_cast<float *>(aligned_base(bad + 4));
    GNNX_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    const float inv_n = 1.0f / (float)n_total;
    // the same choice of form as gnnx_softmax_ce_partial_f32 makes for the same matrix: listing every row gives its dlogits bits
    const bool vec = n_classes % 4 == 0 && n_classes <= 1024 && ldx % 4 == 0 && (!d_dlogits || ldd % 4 == 0) &&
                     (reinterpret_cast<uintptr_t>(d_logits) & 15u) == 0 && (reinterpret_cast<uintptr_t>(d_dlogits) & 15u) == 0;
    float *rl = d_loss ? row_loss : nullptr;
    if (vec) {
        const int groups = ce_groups(n_listed);
        float *cp = d_colsum ? cpart : nullptr;
        const int kv = (n_classes + 255) / 256;
#define GNNX_CE_ROWS_LAUNCH(KV)                                                                                                     \
    hipLaunchKernelGGL(ce_rows_vec_kernel<KV>, dim3((uint32_t)groups), dim3(256), 0, st, d_logits, ldx, d_target, d_rows, n_listed, n_rows, \
                       n_classes, inv_n, rl, d_dlogits, ldd, bad, cp)
        if (kv == 1) GNNX_CE_ROWS_LAUNCH(1);
        else if (kv == 2) GNNX_CE_ROWS_LAUNCH(2);
        else if (kv == 3) GNNX_CE_ROWS_LAUNCH(3);
        else GNNX_CE_ROWS_LAUNCH(4);
#undef GNNX_CE_ROWS_LAUNCH
        GNNX_LAUNCH_CHECK();
        if (d_colsum) {
            hipLaunchKernelGGL(rows_colsum_reduce, dim3((uint32_t)ceil_div(n_classes, 64)), dim3(256), 0, st, cpart, 4 * groups, n_classes,
                               d_colsum);
            GNNX_LAUNCH_CHECK();
        }
    } else {
        hipLaunchKernelGGL(ce_rows_kernel, dim3((uint32_t)ceil_div(n_listed, 4)), dim3(256), 0, st, d_logits, ldx, d_target, d_rows, n_listed,
                           n_rows, n_classes, inv_n, rl, d_dlogits, ldd, bad);
        GNNX_LAUNCH_CHECK();
        if (d_colsum) {
            const int parts = (int)(n_listed < kCeGenericParts ? n_listed : kCeGenericParts);
            const int64_t rpb = ceil_div(n_listed, parts);
            hipLaunchKernelGGL(ce_rows_colsum_generic, dim3((uint32_t)ceil_div(n_classes, 256), (uint32_t)ceil_div(n_listed, rpb)), dim3(256), 0,
                               st, d_dlogits, ldd, d_rows, n_listed, n_rows, n_classes, cpart, rpb);
            GNNX_LAUNCH_CHECK();
            hipLaunchKernelGGL(rows_colsum_reduce, dim3((uint32_t)ceil_div(n_classes, 64)), dim3(256), 0, st, cpart,
                               (int32_t)ceil_div(n_listed, rpb), n_classes, d_colsum);
            GNNX_LAUNCH_CHECK();
        }
    }
    if (d_loss) {
        hipLaunchKernelGGL(rows_sum_stage1, dim3(kSumBlocks), dim3(256), 0, st, row_loss, n_listed, partial);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(rows_sum_stage2, dim3(1), dim3(64), 0, st, partial, kSumBlocks, 1.0f / (float)n_total, d_loss);
        GNNX_LAUNCH_CHECK();
    }
    int32_t h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!(h_bad & 2), GNNX_ERR_INDEX_RANGE, "listed row outside [0, n_rows)");
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "target class out of range at a listed row");
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
