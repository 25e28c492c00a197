// Optimisers over a TABLE of parameter tensors (include/gnnx.h, "optimisers"): Adam / AdamW, SGD with momentum, and the global
// gradient norm for clipping.  A model's parameters are many small tensors (a 256 x 256 weight is 64 chunks of 1024 floats, a bias is
// one), so the update is ONE launch for all of them: one workgroup of 256 threads per chunk, the chunk found from the workgroup id by
// a binary search in the table's prefix array of chunk counts.  The table is built once and lives in device memory:
//     OptimEntry[n_tensors]   { parameter, gradient, element count, offset of the tensor's state in the caller's flat state arena }
//     int32 first[n_tensors + 1]   first[t] = chunks of tensors 0 .. t - 1 (a tensor of size 0 has none: first[t] == first[t + 1])
// No atomics, no host synchronisation and no host-to-device copy in a step.  The arithmetic is the contract of include/gnnx.h: one
// float32 operation with one rounding per line (tests/optim_ref.py restates it; tests/test_gpu_optim.py compares bit patterns).
#include <cmath>
#include <vector>

#include "gnnx_common.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kChunk = 1024;        // elements per workgroup: one float4 per thread
constexpr int kNormBlocks = 256;    // fixed grid of the norm: the partials, and with them every bit, do not depend on the table's size

struct OptimEntry {
    float *p;
    const float *g;
    int64_t n;
    int64_t off;   // elements into the state arena, a multiple of 4
};
static_assert(sizeof(OptimEntry) == 32, "table layout");

size_t table_bytes(int64_t n_tensors) { return ((size_t)n_tensors * sizeof(OptimEntry) + ((size_t)n_tensors + 1) * sizeof(int32_t) + 15u) & ~(size_t)15u; }

__device__ __forceinline__ const int32_t *first_of(const void *table, int32_t n_tensors)
{
    return reinterpret_cast<const int32_t *>(static_cast<const OptimEntry *>(table) + n_tensors);
}

// the tensor of a chunk: the t with first[t] <= chunk < first[t + 1] (chunk < first[n_tensors]); workgroup-uniform
__device__ __forceinline__ int32_t tensor_of(const int32_t *first, int32_t n_tensors, int32_t chunk)
{
    int32_t lo = 0, hi = n_tensors;   // the first index in (0, n_tensors] whose entry is > chunk
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (first[mid + 1] > chunk) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

struct AdamArgs {
    float lr, b1, b2, eps, c1, c2, wd;
    int decoupled;
};

struct MomentumArgs {
    float lr, momentum, dampening, wd;
    int nesterov, first;
};

// g1 = g * s (with a scale), g2 = g1 + wd * p (coupled decay, wd != 0): as sgd_kernel
__device__ __forceinline__ float scaled_decayed(float g, float p, const float *s, float wd, bool coupled)
{
    if (s) g = g * *s;
    if (coupled && wd != 0.f) g = g + wd * p;
    return g;
}

struct AdamOp {
    AdamArgs a;
    float *m, *v;   // the arena
    __device__ __forceinline__ void operator()(float &p, float g, float &m_, float &v_, const float *s) const
    {
        const float g2 = scaled_decayed(g, p, s, a.wd, !a.decoupled);
        const float m1 = a.b1 * m_ + (1.0f - a.b1) * g2;
        const float v1 = a.b2 * v_ + ((1.0f - a.b2) * g2) * g2;
        const float u = (m1 / a.c1) / (sqrtf(v1 / a.c2) + a.eps);
        float p1 = p;
        if (a.decoupled && a.wd != 0.f) p1 = p - (a.lr * a.wd) * p;
        p = p1 - a.lr * u;
        m_ = m1;
        v_ = v1;
    }
};

struct MomentumOp {
    MomentumArgs a;
    float *m, *v;   // m: the momentum buffers; v unused (the same arena pointer)
    __device__ __forceinline__ void operator()(float &p, float g, float &b_, float &, const float *s) const
    {
        const float g2 = scaled_decayed(g, p, s, a.wd, true);
        const float b1 = a.first ? g2 : a.momentum * b_ + (1.0f - a.dampening) * g2;
        const float d = a.nesterov ? g2 + a.momentum * b1 : b1;
        p = p - a.lr * d;
        b_ = b1;
    }
};

// One workgroup per chunk.  float4 lanes where the chunk's parameter, gradient and state addresses are all 16-byte aligned (every
// chunk of a tensor shares the tensor's alignment: 1024 floats are 4 KiB), scalar lanes otherwise; the chunk's tail (< 4 elements on
// the vector form) on scalar lanes either way.  TWO: the op keeps two state vectors (Adam's m and v) or one (the momentum buffer).
template <class Op, bool TWO>
__global__ __launch_bounds__(256) void optim_step_kernel(const void *table, int32_t n_tensors, Op op, const float *gscale)
{
    const int32_t *first = first_of(table, n_tensors);
    const int32_t chunk = (int32_t)blockIdx.x;
    if (chunk >= first[n_tensors]) return;   // a caller's n_chunks above the table's own
    const int32_t t = tensor_of(first, n_tensors, chunk);
    const OptimEntry e = static_cast<const OptimEntry *>(table)[t];
    const int64_t base = (int64_t)(chunk - first[t]) * kChunk;
    const int cnt = (int)(e.n - base < kChunk ? e.n - base : kChunk);
    float *p = e.p + base;
    const float *g = e.g + base;
    float *m = op.m + e.off + base;
    float *v = TWO ? op.v + e.off + base : m;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    const int nvec = vec ? cnt / 4 : 0;   // <= 256
    const int tid = threadIdx.x;
    if (tid < nvec) {
        float4 p4 = reinterpret_cast<float4 *>(p)[tid];
        const float4 g4 = reinterpret_cast<const float4 *>(g)[tid];
        float4 m4 = reinterpret_cast<float4 *>(m)[tid];
        float4 v4 = TWO ? reinterpret_cast<float4 *>(v)[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        op(p4.x, g4.x, m4.x, v4.x, gscale);
        op(p4.y, g4.y, m4.y, v4.y, gscale);
        op(p4.z, g4.z, m4.z, v4.z, gscale);
        op(p4.w, g4.w, m4.w, v4.w, gscale);
        reinterpret_cast<float4 *>(p)[tid] = p4;
        reinterpret_cast<float4 *>(m)[tid] = m4;
        if (TWO) reinterpret_cast<float4 *>(v)[tid] = v4;
    }
    for (int i = 4 * nvec + tid; i < cnt; i += 256) {
        float pi = p[i], mi = m[i], vi = TWO ? v[i] : 0.f;
        op(pi, g[i], mi, vi, gscale);
        p[i] = pi;
        m[i] = mi;
        if (TWO) v[i] = vi;
    }
}

// ---- the squared norm of every gradient of the table: the scheme of the loss kernels (gnnx_train.hip) --------------------------------
// A fixed grid strides the chunks; thread i of a workgroup adds elements i, i + 256, i + 512, i + 768 of each of its chunks in that
// order (scalar loads whatever the alignment: the order, and so the bits, do not depend on where a gradient sits); a fixed tree
// folds the 256 sums; stage 2 adds the kNormBlocks partials in order.  The same bits on every run.
__global__ __launch_bounds__(256) void sqnorm_stage1(const void *table, int32_t n_tensors, float *partial)
{
    __shared__ float red[256];
    const int32_t *first = first_of(table, n_tensors);
    const int32_t n_chunks = first[n_tensors];
    float acc = 0.f;
    for (int32_t chunk = (int32_t)blockIdx.x; chunk < n_chunks; chunk += kNormBlocks) {
        const int32_t t = tensor_of(first, n_tensors, chunk);
        const OptimEntry e = static_cast<const OptimEntry *>(table)[t];
        const int64_t base = (int64_t)(chunk - first[t]) * kChunk;
        const int cnt = (int)(e.n - base < kChunk ? e.n - base : kChunk);
        const float *g = e.g + base;
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const float gi = g[i];
            acc += gi * gi;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void sqnorm_stage2(const float *partial, float max_norm, float *sqnorm, float *gscale)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float acc = 0.f;
        for (int b = 0; b < kNormBlocks; b++) acc += partial[b];
        if (sqnorm) *sqnorm = acc;
        if (gscale) {
            const float q = max_norm / (sqrtf(acc) + 1e-6f);
            *gscale = q > 1.0f ? 1.0f : q;   // min(1, q) that keeps a NaN (torch's clamp(max = 1))
        }
    }
}

int check_step(const void *table, int32_t n_tensors, int64_t n_chunks, const void *state)
{
    GNNX_REQUIRE(n_tensors >= 0 && n_chunks >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_chunks < ((int64_t)1 << 31), GNNX_ERR_UNSUPPORTED, "%lld chunks: 2^31 or more", (long long)n_chunks);
    GNNX_REQUIRE(table && (reinterpret_cast<uintptr_t>(table) & 7u) == 0, GNNX_ERR_INVALID_ARG, "table is null or not 8-byte aligned");
    GNNX_REQUIRE(n_chunks == 0 || state, GNNX_ERR_INVALID_ARG, "state arena is null");
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_optim_table_bytes(int32_t n_tensors, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_tensors >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = table_bytes(n_tensors);
    return GNNX_OK;
}

GNNX_API int gnnx_optim_table_build(int32_t n_tensors, float *const *h_params, const float *const *h_grads, const int64_t *h_sizes,
                                    void *d_table, size_t table_bytes_given, int64_t *n_chunks_out, int64_t *state_elems_out, void *stream)
{
    GNNX_REQUIRE(n_tensors >= 0, GNNX_ERR_INVALID_ARG, "negative tensor count");
    GNNX_REQUIRE(n_tensors == 0 || (h_params && h_grads && h_sizes), GNNX_ERR_INVALID_ARG, "null host array");
    GNNX_REQUIRE(n_chunks_out && state_elems_out, GNNX_ERR_INVALID_ARG, "null output");
    const size_t need = table_bytes(n_tensors);
    std::vector<char> host(need, 0);
    OptimEntry *e = reinterpret_cast<OptimEntry *>(host.data());
    int32_t *first = reinterpret_cast<int32_t *>(e + n_tensors);
    int64_t chunks = 0, off = 0;
    for (int32_t t = 0; t < n_tensors; t++) {
        const int64_t n = h_sizes[t];
        GNNX_REQUIRE(n >= 0, GNNX_ERR_INVALID_ARG, "tensor %d: negative size", t);
        GNNX_REQUIRE(n == 0 || (h_params[t] && h_grads[t]), GNNX_ERR_INVALID_ARG, "tensor %d: null parameter or gradient", t);
        GNNX_REQUIRE(n == 0 || ((reinterpret_cast<uintptr_t>(h_params[t]) | reinterpret_cast<uintptr_t>(h_grads[t])) & 3u) == 0, GNNX_ERR_INVALID_ARG,
                     "tensor %d: pointer not 4-byte aligned", t);
        GNNX_REQUIRE(n <= INT64_MAX - 3 - off, GNNX_ERR_UNSUPPORTED, "state arena beyond 2^63 elements");
        first[t] = (int32_t)chunks;
        e[t] = OptimEntry{h_params[t], h_grads[t], n, off};
        chunks += ceil_div(n, kChunk);
        GNNX_REQUIRE(chunks < ((int64_t)1 << 31), GNNX_ERR_UNSUPPORTED, "2^31 or more chunks of %d elements", kChunk);
        off += (n + 3) & ~(int64_t)3;   // every tensor's state starts on a 16-byte boundary of the arena
    }
    first[n_tensors] = (int32_t)chunks;
    GNNX_REQUIRE(d_table && (reinterpret_cast<uintptr_t>(d_table) & 7u) == 0, GNNX_ERR_INVALID_ARG, "table is null or not 8-byte aligned");
    GNNX_REQUIRE(table_bytes_given >= need, GNNX_ERR_WORKSPACE, "table %zu < required %zu", table_bytes_given, need);
    hipStream_t st = as_stream(stream);
    GNNX_HIP_CHECK(hipMemcpyAsync(d_table, host.data(), need, hipMemcpyHostToDevice, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));   // the staging copy lives on this frame: a build call, not a per-step one
    *n_chunks_out = chunks;
    *state_elems_out = off;
    return GNNX_OK;
}

GNNX_API int gnnx_adam_bias_corrections(float b1, float b2, int64_t t, float *c1, float *c2)
{
    GNNX_REQUIRE(c1 && c2 && t >= 1, GNNX_ERR_INVALID_ARG, "null output or step count < 1");
    GNNX_REQUIRE(b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f, GNNX_ERR_INVALID_ARG, "beta outside [0, 1)");
    *c1 = (float)(1.0 - pow((double)b1, (double)t));
    *c2 = (float)(1.0 - pow((double)b2, (double)t));
    return GNNX_OK;
}

GNNX_API int gnnx_adam_step_f32(const void *d_table, int32_t n_tensors, int64_t n_chunks, float *d_m, float *d_v, float lr, float b1, float b2,
                                float eps, float c1, float c2, float weight_decay, int decoupled, const float *d_gscale, void *stream)
{
    const int rc = check_step(d_table, n_tensors, n_chunks, d_m);
    if (rc != GNNX_OK) return rc;
    GNNX_REQUIRE(n_chunks == 0 || d_v, GNNX_ERR_INVALID_ARG, "state arena is null");
    GNNX_REQUIRE(b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f, GNNX_ERR_INVALID_ARG, "beta outside [0, 1)");
    GNNX_REQUIRE(eps > 0.f, GNNX_ERR_INVALID_ARG, "eps <= 0");
    GNNX_REQUIRE(c1 > 0.f && c2 > 0.f, GNNX_ERR_INVALID_ARG, "bias correction <= 0");
    if (n_chunks == 0) return GNNX_OK;
    const AdamOp op{AdamArgs{lr, b1, b2, eps, c1, c2, weight_decay, decoupled != 0}, d_m, d_v};
    hipLaunchKernelGGL((optim_step_kernel<AdamOp, true>), dim3((uint32_t)n_chunks), dim3(256), 0, as_stream(stream), d_table, n_tensors, op, d_gscale);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_momentum_step_f32(const void *d_table, int32_t n_tensors, int64_t n_chunks, float *d_buf, float lr, float momentum,
                                    float dampening, int nesterov, int first, float weight_decay, const float *d_gscale, void *stream)
{
    const int rc = check_step(d_table, n_tensors, n_chunks, d_buf);
    if (rc != GNNX_OK) return rc;
    if (n_chunks == 0) return GNNX_OK;
    const MomentumOp op{MomentumArgs{lr, momentum, dampening, weight_decay, nesterov != 0, first != 0}, d_buf, d_buf};
    hipLaunchKernelGGL((optim_step_kernel<MomentumOp, false>), dim3((uint32_t)n_chunks), dim3(256), 0, as_stream(stream), d_table, n_tensors, op,
                       d_gscale);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_grad_sqnorm_workspace(size_t *bytes)
{
    GNNX_REQUIRE(bytes, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = sizeof(float) * kNormBlocks;
    return GNNX_OK;
}

GNNX_API int gnnx_grad_sqnorm_f32(const void *d_table, int32_t n_tensors, float max_norm, float *d_sqnorm, float *d_gscale, void *d_workspace,
                                  size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_tensors >= 0, GNNX_ERR_INVALID_ARG, "negative tensor count");
    GNNX_REQUIRE(d_table && (reinterpret_cast<uintptr_t>(d_table) & 7u) == 0, GNNX_ERR_INVALID_ARG, "table is null or not 8-byte aligned");
    GNNX_REQUIRE(d_sqnorm || d_gscale, GNNX_ERR_INVALID_ARG, "both outputs are null");
    GNNX_REQUIRE(!d_gscale || max_norm >= 0.f, GNNX_ERR_INVALID_ARG, "max_norm is negative or NaN");
    GNNX_REQUIRE(d_workspace && workspace_bytes >= sizeof(float) * kNormBlocks && (reinterpret_cast<uintptr_t>(d_workspace) & 3u) == 0,
                 GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, sizeof(float) * kNormBlocks);
    hipStream_t st = as_stream(stream);
    float *partial = static_cast<float *>(d_workspace);
    hipLaunchKernelGGL(sqnorm_stage1, dim3(kNormBlocks), dim3(256), 0, st, d_table, n_tensors, partial);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sqnorm_stage2, dim3(1), dim3(64), 0, st, partial, max_norm, d_sqnorm, d_gscale);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}
