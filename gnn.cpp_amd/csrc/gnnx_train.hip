// Training-step pieces around the hot path: softmax cross-entropy on the logits of the
// last GCN layer and the SGD parameter update, so a 2/3-layer GCN runs as a whole training step on the device.
//   loss   (reference nn.cpp:442-453, forward only -- its backward throws):  l_i = -log( exp(x_i[t_i]) / (sum_c exp(x_ic) + 1e-20) ),
//          loss = (sum_i l_i) / N.   No max-subtraction, like the reference (logits of a GCN layer are O(1..100)).
//   dlogits (textbook; the reference has none that works):  (softmax(x_i) - onehot(t_i)) / N
//   SGD    (textbook; the reference's step() reads an empty velocity vector, nn.cpp:414):  p -= lr * (g + wd * p)
// Error bounds of the loss (include/gnnx.h; u = 2^-24, S = 4 ceil(C / 256) + 6 additions on the row sum of the vector form,
// ceil(C / 64) + 6 on the generic walk): gradient (S + 8) u (p + onehot) / N, column sums (S + 8 + n) u sum (p + onehot) / N,
// loss u [(S + 4) n + (ceil(n / 65536) + 266) sum |l_i|] / N.  Worst ratios error / (u * scale) that tests/test_gpu_loss.py has seen
// on an MI355X:  vector form  gradient 5.3, column sums 5.4, loss 3.5 (of u sum |l_i| / N; 1.3 % of its bound)
//                generic      gradient 5.4, column sums 4.4, loss 3.2
//                BCE          gradient 3.4 (bound 6), loss 1.4 (bound 276)
// On inputs where nothing rounds (logits 0 or dead, 1 / 2 / 4 / 8 live classes, N a power of two) every path is exact to the bit.
#include "gnnx_common.h"

#include <type_traits>

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

// Which rows a loss kernel works on: all n of them (work item i is row i), or the n entries of a row list (work item i is row
// rows[i], held against [0, n_rows)).  The plain form carries the count alone: its kernels have no list operand and no check.
template <bool LISTED>
struct RowSel;
template <>
struct RowSel<false> {
    int64_t n;
};
template <>
struct RowSel<true> {
    int64_t n;
    const int32_t *rows;
    int64_t n_rows;
};

// one wavefront per work item: lanes stride the classes; per-item loss to slot i of a buffer, gradient written in place
template <bool LISTED>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float *X, int64_t ldx, const int32_t *target, RowSel<LISTED> sel,
                                                          int32_t n_cls, float inv_n, float *row_loss, float *dX, int64_t ldd,
                                                          int32_t *bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= sel.n) return;
    int64_t row = i;
    if constexpr (LISTED) {
        row = sel.rows[i];
        if (row < 0 || row >= sel.n_rows) {   // wave-uniform
            if (lane == 0) atomicOr(bad, 2);
            return;
        }
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

// Vector form for class counts that are a multiple of 4 and at most 1024 (row stride a multiple of 4, 16-byte aligned): one
// wavefront per row, a lane holds classes 256 k + 4 lane .. + 3 (one 16-byte load per k: a 256-class row is ONE 1-KiB
// wave-instruction), exp evaluated once per element and kept in registers, two rows in flight per wavefront.  Waves walk the work
// items with a grid stride; with `colsum_partial` a wavefront also keeps the column sums of the gradient rows it wrote -- the last
// layer's bias gradient, which otherwise is one more 4 N C-byte pass -- and stores them as row `wave id` of the partials (summed
// by ce_colsum_reduce in a fixed order: deterministic).  Same expressions per element as the generic kernel above
// (expf(x) * (1 / (sum + 1e-20)), then - onehot, then * 1/N); only the ORDER of the row sum differs (tolerance-level, as documented).
template <int KV, bool LISTED>
__global__ __launch_bounds__(256) void softmax_ce_vec_kernel(const float *X, int64_t ldx, const int32_t *target, RowSel<LISTED> sel,
                                                              int32_t n_cls, float inv_n, float *row_loss, float *dX, int64_t ldd,
                                                              int32_t *bad, float *colsum_partial)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    float4 cs[KV];
#pragma unroll
    for (int k = 0; k < KV; k++) cs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i0 = wave; i0 < sel.n; i0 += 2 * n_waves) {
        float4 e[2][KV];
        int32_t t[2];
        int64_t listed[2];   // LISTED: rows[i], loaded once
        bool have[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int64_t i = i0 + u * n_waves;
            have[u] = i < sel.n;
            int64_t row = i;
            if constexpr (LISTED) {
                row = have[u] ? (int64_t)sel.rows[i] : 0;
                if (have[u] && (row < 0 || row >= sel.n_rows)) {   // wave-uniform
                    if (lane == 0) atomicOr(bad, 2);
                    have[u] = false;
                }
                listed[u] = row;
            }
            t[u] = have[u] ? target[row] : 0;
#pragma unroll
            for (int k = 0; k < KV; k++) {
                const int32_t c = 256 * k + 4 * lane;
                e[u][k] = (have[u] && c < n_cls) ? *reinterpret_cast<const float4 *>(X + row * ldx + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (!have[u]) continue;   // wave-uniform
            const int64_t row = LISTED ? listed[u] : i0 + u * n_waves;
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
            if (lane == 0 && row_loss) row_loss[i0 + u * n_waves] = -logf(expf(X[row * ldx + t[u]]) / denom);
            if (dX) {
                const float rden = 1.0f / denom;   // the gradient has no reference arithmetic to follow (its backward throws): one
                                                   // division per row, a multiplication per element
#pragma unroll
                for (int k = 0; k < KV; k++) {
                    const int32_t c = 256 * k + 4 * lane;
                    if (c < n_cls) {
                        float4 d;
                        d.x = (e[u][k].x * rden - (c + 0 == t[u] ? 1.f : 0.f)) * inv_n;
                        d.y = (e[u][k].y * rden - (c + 1 == t[u] ? 1.f : 0.f)) * inv_n;
                        d.z = (e[u][k].z * rden - (c + 2 == t[u] ? 1.f : 0.f)) * inv_n;
                        d.w = (e[u][k].w * rden - (c + 3 == t[u] ? 1.f : 0.f)) * inv_n;
                        *reinterpret_cast<float4 *>(dX + row * ldd + c) = d;
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

// out[c] = sum over the partial rows, 4 interleaved parts per column combined in part order (fixed order: deterministic)
__global__ __launch_bounds__(256) void ce_colsum_reduce(const float *partial, int32_t n_part, int32_t n_cls, float *out)
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

// generic class counts: a lane walks the classes with stride 64; the column sums (when asked for) by one thread per class
// over the finished gradient rows of a block of the work items (a second pass; only for shapes off the vector form).  A listed
// row outside the matrix was refused by the loss kernel and is skipped here.
template <bool LISTED>
__global__ __launch_bounds__(256) void ce_colsum_generic(const float *dX, int64_t ldd, RowSel<LISTED> sel, int32_t n_cls, float *partial,
                                                          int64_t rows_per_block)
{
    const int64_t i0 = (int64_t)blockIdx.y * rows_per_block, i1 = i0 + rows_per_block < sel.n ? i0 + rows_per_block : sel.n;
    const int32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cls) return;
    float acc = 0.f;
    for (int64_t i = i0; i < i1; i++) {
        int64_t row = i;
        if constexpr (LISTED) {
            row = sel.rows[i];
            if (row < 0 || row >= sel.n_rows) continue;
        }
        acc += dX[row * ldd + c];
    }
    partial[(int64_t)blockIdx.y * n_cls + c] = acc;
}

// deterministic two-stage mean of the per-row losses
__global__ __launch_bounds__(256) void sum_stage1(const float *v, int64_t n, float *partial)
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
__global__ void sum_stage2(const float *partial, int n_blocks, float scale, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float acc = 0.f;
        for (int b = 0; b < n_blocks; b++) acc += partial[b];
        *out = acc * scale;
    }
}

__global__ __launch_bounds__(256) void sgd_kernel(float *p, const float *g, int64_t n, float lr, float wd)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float gi = g[i];
        if (wd != 0.f) gi = gi + wd * p[i];
        p[i] = p[i] - lr * gi;
    }
}

constexpr int kSumBlocks = 256;
constexpr int kCeMaxGroups = 2048;   // vector form: at most this many workgroups of 4 wavefronts (8 per CU)
constexpr int kCeGenericParts = 256;

inline int ce_groups(int64_t n_rows)
{
    int64_t gsz = ceil_div(n_rows, 8);   // 4 wavefronts, 2 rows in flight each
    return (int)(gsz < 1 ? 1 : (gsz > kCeMaxGroups ? kCeMaxGroups : gsz));
}

// the caller's workspace, carved: row_loss[n_listed] | partial[kSumBlocks] | bad | column-sum partials (256-byte aligned; only with
// want_colsum: a row per wavefront of the vector form or per block of the generic pass)
struct CeWs {
    float *row_loss, *partial, *cpart;
    int32_t *bad;
};

// bytes the loss needs; with `base` (any alignment) also the layout in *out
size_t carve(int64_t n_listed, int32_t n_classes, bool want_colsum, void *base, CeWs *out)
{
    Carver c(base ? aligned_base(base) : nullptr);
    CeWs w{};
    w.row_loss = c.take<float>((size_t)n_listed, 4);
    w.partial = c.take<float>(kSumBlocks, 4);
    w.bad = c.take<int32_t>(1, 4);
    const size_t parts = (size_t)(4 * ce_groups(n_listed) > kCeGenericParts ? 4 * ce_groups(n_listed) : kCeGenericParts);
    float *cpart = c.take<float>(want_colsum ? parts * (size_t)n_classes : 0, 256);
    if (want_colsum) w.cpart = cpart;
    if (out) *out = w;
    return c.off + 256;   // room to align the caller's pointer (the end of cpart is not rounded up: the count callers have always got)
}

// The loss over every row of the matrix (rows == nullptr: n_listed == n_rows) or over the listed rows, divisor n_total: the same
// kernels, grids and summation orders either way, so listing every row gives the bits of the plain call.
int softmax_ce(const float *logits, int64_t ldx, const int32_t *target, const int32_t *rows /* null: every row */, int64_t n_listed,
               int64_t n_rows, int32_t n_classes, int64_t n_total, float *loss, float *dlogits, int64_t ldd, float *colsum, void *workspace,
               size_t bytes, void *stream)
{
    GNNX_REQUIRE(n_listed > 0 && n_classes > 0, GNNX_ERR_INVALID_ARG, "empty batch");
    GNNX_REQUIRE(n_rows >= n_listed, GNNX_ERR_INVALID_ARG, "more listed rows than rows");
    GNNX_REQUIRE(n_total >= n_listed, GNNX_ERR_INVALID_ARG, "n_total < number of rows in the loss");
    GNNX_REQUIRE(logits && target && ldx >= n_classes, GNNX_ERR_INVALID_ARG, "null pointer or ld < n_classes");
    GNNX_REQUIRE(!dlogits || ldd >= n_classes, GNNX_ERR_INVALID_ARG, "ldd < n_classes");
    GNNX_REQUIRE(!colsum || dlogits, GNNX_ERR_INVALID_ARG, "column sums are those of dlogits: dlogits is null");
    CeWs w;
    const size_t need = carve(n_listed, n_classes, colsum != nullptr, workspace, &w);
    GNNX_REQUIRE(workspace && bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", bytes, need);
    hipStream_t st = as_stream(stream);
    GNNX_HIP_CHECK(hipMemsetAsync(w.bad, 0, sizeof(int32_t), st));
    const float inv_n = 1.0f / (float)n_total;
    float *rl = loss ? w.row_loss : nullptr;
    const bool vec = n_classes % 4 == 0 && n_classes <= 1024 && ldx % 4 == 0 && (!dlogits || ldd % 4 == 0) && aligned16(logits) &&
                     aligned16(dlogits);
    auto launch = [&](auto sel) -> int {
        constexpr bool LISTED = std::is_same_v<decltype(sel), RowSel<true>>;
        int32_t n_part;   // rows of the column-sum partials
        if (vec) {
            const int groups = ce_groups(n_listed);
            n_part = 4 * groups;
#define GNNX_CE_LAUNCH(KV)                                                                                                              \
    hipLaunchKernelGGL((softmax_ce_vec_kernel<KV, LISTED>), dim3((uint32_t)groups), dim3(256), 0, st, logits, ldx, target, sel, n_classes, \
                       inv_n, rl, dlogits, ldd, w.bad, w.cpart)
            const int kv = (n_classes + 255) / 256;
            if (kv == 1) GNNX_CE_LAUNCH(1);
            else if (kv == 2) GNNX_CE_LAUNCH(2);
            else if (kv == 3) GNNX_CE_LAUNCH(3);
            else GNNX_CE_LAUNCH(4);
#undef GNNX_CE_LAUNCH
            GNNX_LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(softmax_ce_kernel<LISTED>, dim3((uint32_t)ceil_div(n_listed, 4)), dim3(256), 0, st, logits, ldx, target, sel,
                               n_classes, inv_n, rl, dlogits, ldd, w.bad);
            GNNX_LAUNCH_CHECK();
            const int parts = (int)(n_listed < kCeGenericParts ? n_listed : kCeGenericParts);
            const int64_t rpb = ceil_div(n_listed, parts);
            n_part = (int32_t)ceil_div(n_listed, rpb);
            if (colsum) {
                hipLaunchKernelGGL(ce_colsum_generic<LISTED>, dim3((uint32_t)ceil_div(n_classes, 256), (uint32_t)n_part), dim3(256), 0, st,
                                   dlogits, ldd, sel, n_classes, w.cpart, rpb);
                GNNX_LAUNCH_CHECK();
            }
        }
        if (colsum) {
            hipLaunchKernelGGL(ce_colsum_reduce, dim3((uint32_t)ceil_div(n_classes, 64)), dim3(256), 0, st, w.cpart, n_part, n_classes, colsum);
            GNNX_LAUNCH_CHECK();
        }
        return GNNX_OK;
    };
    const int status = rows ? launch(RowSel<true>{n_listed, rows, n_rows}) : launch(RowSel<false>{n_listed});
    if (status != GNNX_OK) return status;
    if (loss) {
        hipLaunchKernelGGL(sum_stage1, dim3(kSumBlocks), dim3(256), 0, st, w.row_loss, n_listed, w.partial);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(64), 0, st, w.partial, kSumBlocks, 1.0f / (float)n_total, loss);
        GNNX_LAUNCH_CHECK();
    }
    int32_t h_bad = 0;
    GNNX_HIP_CHECK(hipMemcpyAsync(&h_bad, w.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!(h_bad & 2), GNNX_ERR_INDEX_RANGE, "listed row outside [0, n_rows)");
    GNNX_REQUIRE(!h_bad, GNNX_ERR_INDEX_RANGE, "target class out of range");
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_softmax_ce_colsum_workspace(int64_t n_rows, int32_t n_classes, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_rows >= 0 && n_classes >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = carve(n_rows, n_classes, true, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_softmax_ce_workspace(int64_t n_rows, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_rows >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = carve(n_rows, 0, false, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_softmax_ce_rows_workspace(int64_t n_listed, int32_t n_classes, size_t *bytes)
{
    return gnnx_softmax_ce_colsum_workspace(n_listed, n_classes, bytes);
}

// A shard's share of the loss over n_total rows: the mean's divisor is n_total (>= n_rows), so d_loss is THIS rank's term of the
// mean (summed over the ranks by the caller) and dlogits / the column sums carry 1 / n_total -- the same expression per element as
// the unsharded call with n_total rows.
GNNX_API int gnnx_softmax_ce_partial_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, int64_t n_rows, int32_t n_classes,
                                         int64_t n_total, float *d_loss, float *d_dlogits, int64_t ldd, float *d_colsum,
                                         void *d_workspace, size_t workspace_bytes, void *stream)
{
    return softmax_ce(d_logits, ldx, d_target, nullptr, n_rows, n_rows, n_classes, n_total, d_loss, d_dlogits, ldd, d_colsum, d_workspace,
                      workspace_bytes, stream);
}

GNNX_API int gnnx_softmax_ce_colsum_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, int64_t n_rows, int32_t n_classes,
                                        float *d_loss, float *d_dlogits, int64_t ldd, float *d_colsum, void *d_workspace,
                                        size_t workspace_bytes, void *stream)
{
    return gnnx_softmax_ce_partial_f32(d_logits, ldx, d_target, n_rows, n_classes, n_rows, d_loss, d_dlogits, ldd, d_colsum, d_workspace,
                                       workspace_bytes, stream);
}

GNNX_API int gnnx_softmax_ce_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, int64_t n_rows, int32_t n_classes,
                                 float *d_loss, float *d_dlogits, int64_t ldd, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return gnnx_softmax_ce_colsum_f32(d_logits, ldx, d_target, n_rows, n_classes, d_loss, d_dlogits, ldd, nullptr, d_workspace,
                                      workspace_bytes, stream);
}

// The same loss over the rows a list names (semi-supervised training, include/gnnx.h): work item i is row d_rows[i], only listed
// rows of dlogits are written, d_target is read at listed rows only; cost O(n_listed).
GNNX_API int gnnx_softmax_ce_rows_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, const int32_t *d_rows, int64_t n_listed,
                                      int64_t n_rows, int32_t n_classes, int64_t n_total, float *d_loss, float *d_dlogits, int64_t ldd,
                                      float *d_colsum, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_listed > 0, GNNX_ERR_INVALID_ARG, "empty row list (the mean over no rows is undefined)");
    GNNX_REQUIRE(d_rows, GNNX_ERR_INVALID_ARG, "null row list");
    return softmax_ce(d_logits, ldx, d_target, d_rows, n_listed, n_rows, n_classes, n_total, d_loss, d_dlogits, ldd, d_colsum, d_workspace,
                      workspace_bytes, stream);
}

GNNX_API int gnnx_sgd_step_f32(float *d_param, const float *d_grad, int64_t n, float lr, float weight_decay, void *stream)
{
    GNNX_REQUIRE(n >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    if (n == 0) return GNNX_OK;
    GNNX_REQUIRE(d_param && d_grad, GNNX_ERR_INVALID_ARG, "null pointer");
    int64_t blocks = ceil_div(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sgd_kernel, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), d_param, d_grad, n, lr, weight_decay);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

// ---- binary cross-entropy on logits: the loss over scored pairs (link prediction; include/gnnx.h) --------------------------------
//   l_p = max(x, 0) - x * y + log1p(exp(-|x|))          the stable form: exp never sees a positive argument, no inf / NaN for any
//                                                        finite x (x = +-100: l = 100 or 0 up to exp(-100))
//   ds_p = (sigmoid(x) - y) / n_total,  sigmoid from exp(-|x|) as well
// One pass: a fixed grid of kSumBlocks workgroups strides the entries, a thread adds its terms in index order, the workgroup folds
// its 256 sums in a fixed tree, sum_stage2 adds the kSumBlocks partials in order (the scheme of the softmax loss above and of
// gnnx_colsum_f32: the same bits on every run).
namespace {

__global__ __launch_bounds__(256) void bce_logits_kernel(const float *x, const float *y, int64_t n, float inv_n, float *partial, float *dx)
{
    __shared__ float red[256];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float xi = x[i], yi = y[i];
        const float e = expf(-fabsf(xi));   // in (0, 1]
        if (partial) acc += (fmaxf(xi, 0.f) - xi * yi) + log1pf(e);
        if (dx) {
            const float sig = xi >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
            dx[i] = (sig - yi) * inv_n;
        }
    }
    if (!partial) return;
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

}  // namespace

GNNX_API int gnnx_bce_logits_workspace(int64_t n, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = sizeof(float) * kSumBlocks;
    return GNNX_OK;
}

GNNX_API int gnnx_bce_logits_f32(const float *d_scores, const float *d_target, int64_t n, int64_t n_total, float *d_loss, float *d_dscores,
                                 void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n > 0, GNNX_ERR_INVALID_ARG, "empty score list");
    GNNX_REQUIRE(n_total >= n, GNNX_ERR_INVALID_ARG, "n_total < n");
    GNNX_REQUIRE(d_scores && d_target, GNNX_ERR_INVALID_ARG, "null pointer");
    if (!d_loss && !d_dscores) return GNNX_OK;
    GNNX_REQUIRE(!d_loss || (d_workspace && workspace_bytes >= sizeof(float) * kSumBlocks), GNNX_ERR_WORKSPACE, "workspace %zu < required %zu",
                 workspace_bytes, sizeof(float) * kSumBlocks);
    hipStream_t st = as_stream(stream);
    float *partial = d_loss ? static_cast<float *>(d_workspace) : nullptr;
    const float inv_n = 1.0f / (float)n_total;
    hipLaunchKernelGGL(bce_logits_kernel, dim3(kSumBlocks), dim3(256), 0, st, d_scores, d_target, n, inv_n, partial, d_dscores);
    GNNX_LAUNCH_CHECK();
    if (d_loss) {
        hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(64), 0, st, partial, kSumBlocks, inv_n, d_loss);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}
