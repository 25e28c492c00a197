// BatchNorm (training-mode batch statistics) + ReLU between the transform and the aggregation of GCNConv::forward
// (reference graph.cpp:174-175 -> nn.cpp:285-330 BatchNorm::forward, nn.cpp:229-237 ReLU::forward) -- the first
// "next" row of SURVEY.md section 8(f).  HBM-bound streaming kernels:
//   stats    mean_f = (1/N) sum_i x_if ;  var_f = (1/N) sum_i (x_if - mean_f)^2   (x->mean(-2), x->var(-2, correction 0))
//   forward  y = relu( ((x - mean) / (var + eps)^0.5) * gamma + beta )             each op separately rounded, in the
//            reference's order (sub, div, mul, add); relu = where(x > 0, x, 0)
//   backward (mathematically correct; the reference's own is fan-in-dropping, operation.h:82-86):
//            g = dY * (y > 0);  dbeta = sum g;  dgamma = sum g * xhat;  dx = (gamma / sigma) * (g - dbeta/N - xhat * dgamma/N)
// Column reductions use a fixed grid + fixed combine order (deterministic).
#include "gnnx_common.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kBlocks = 1024;

// Generic column reduction of up to two per-element terms.  Thread -> (row slot rr, column f) with fw columns per
// pass; rows of the workgroup's slab are walked by the slots interleaved, 4 in flight; slots combined through LDS.
template <class OP>
__global__ __launch_bounds__(256) void colreduce_stage1(OP op, int64_t n_rows, int32_t n_feat, int32_t fw, int64_t rows_per_block,
                                                         float *partial0, float *partial1)
{
    __shared__ float red0[256], red1[256];
    const int rpp = 256 / fw;
    const int c = threadIdx.x % fw, rr = threadIdx.x / fw;
    int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    for (int32_t f0 = 0; f0 < n_feat; f0 += fw) {
        const int32_t f = f0 + c;
        float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
        if (f < n_feat && rr < rpp) {
            int64_t r = r0 + rr;
            for (; r + 3 * (int64_t)rpp < r1; r += 4 * (int64_t)rpp) {
#pragma unroll
                for (int u = 0; u < 4; u++) op.term(r + u * (int64_t)rpp, f, a0[u], a1[u]);
            }
            for (; r < r1; r += rpp) op.term(r, f, a0[0], a1[0]);
        }
        red0[threadIdx.x] = (a0[0] + a0[1]) + (a0[2] + a0[3]);
        if (OP::kTwo) red1[threadIdx.x] = (a1[0] + a1[1]) + (a1[2] + a1[3]);
        __syncthreads();
        if (rr == 0 && f < n_feat) {
            float s0 = 0.f, s1 = 0.f;
            for (int k = 0; k < rpp; k++) {
                s0 += red0[k * fw + c];
                if (OP::kTwo) s1 += red1[k * fw + c];
            }
            partial0[(int64_t)blockIdx.x * n_feat + f] = s0;
            if (OP::kTwo) partial1[(int64_t)blockIdx.x * n_feat + f] = s1;
        }
        __syncthreads();
    }
}

// out[f] = scale * sum_b partial[b][f]
__global__ __launch_bounds__(256) void colreduce_stage2(const float *partial, int32_t n_blocks, int32_t n_feat, float scale, float *out)
{
    __shared__ float red[256];
    const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int32_t f = blockIdx.x * 64 + c;
    float acc = 0.f;
    if (f < n_feat)
        for (int32_t b = part; b < n_blocks; b += 4) acc += partial[(int64_t)b * n_feat + f];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (part == 0 && f < n_feat) out[f] = (((red[c] + red[64 + c]) + red[128 + c]) + red[192 + c]) * scale;
}

struct OpIdent {
    static constexpr bool kTwo = false;
    const float *X;
    int64_t ldx;
    __device__ __forceinline__ void term(int64_t r, int32_t f, float &a0, float &) const { a0 += X[r * ldx + f]; }
};
struct OpSqDev {
    static constexpr bool kTwo = false;
    const float *X;
    int64_t ldx;
    const float *mean;
    __device__ __forceinline__ void term(int64_t r, int32_t f, float &a0, float &) const
    {
        float d = X[r * ldx + f] - mean[f];
        a0 += d * d;
    }
};
// Did the forward ReLU pass this element?  From the saved forward output when there is one; otherwise (fused forward,
// gnnx_spmm_csr_fused_f32: the rectified activations were never stored) by redoing the forward arithmetic on x.
__device__ __forceinline__ bool relu_passed(const float *Y, int64_t yi, float x, int32_t f, const float *mean, const float *var, float eps,
                                            const float *gamma, const float *beta)
{
    if (Y) return Y[yi] > 0.f;
    float v = x;
    if (mean) {
        v = __fdiv_rn(__fsub_rn(v, mean[f]), sqrtf(__fadd_rn(var[f], eps)));
        if (gamma) v = __fmul_rn(v, gamma[f]);
        if (beta) v = __fadd_rn(v, beta[f]);
    }
    return v > 0.f;
}

// g = dY * (Y > 0 or no relu);  sums of g and of g * xhat
struct OpBnBwd {
    static constexpr bool kTwo = true;
    const float *X, *Y, *dY, *mean, *rstd;
    int64_t ldx, ldy, ldd;
    int relu;
    const float *var, *gamma, *beta;
    float eps;
    __device__ __forceinline__ void term(int64_t r, int32_t f, float &a0, float &a1) const
    {
        float g = dY[r * ldd + f];
        const float x = X[r * ldx + f];
        if (relu && !relu_passed(Y, r * ldy + f, x, f, mean, var, eps, gamma, beta)) g = 0.f;
        float xhat = (x - mean[f]) * rstd[f];
        a0 += g;
        a1 += g * xhat;
    }
};

__global__ __launch_bounds__(256) void bn_fwd_kernel(const float *X, int64_t ldx, int64_t n_rows, int32_t n_feat, const float *mean,
                                                      const float *var, float eps, const float *gamma, const float *beta, int relu,
                                                      float *Y, int64_t ldy)
{
    int64_t total = n_rows * n_feat;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t r = i / n_feat;
        int32_t f = (int32_t)(i - r * n_feat);
        float v = X[r * ldx + f];
        if (mean) {
            float sd = sqrtf(__fadd_rn(var[f], eps));           // (var + eps)->pow(0.5)
            v = __fdiv_rn(__fsub_rn(v, mean[f]), sd);             // (x - mean) / sd
            if (gamma) v = __fmul_rn(v, gamma[f]);                // * gammas
            if (beta) v = __fadd_rn(v, beta[f]);                  // + betas
        }
        if (relu) v = v > 0.f ? v : 0.f;                          // where(x > 0, x, 0)
        Y[r * ldy + f] = v;
    }
}

__global__ __launch_bounds__(256) void rstd_kernel(const float *var, float eps, int32_t n_feat, float *rstd)
{
    int32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_feat) rstd[f] = 1.0f / sqrtf(var[f] + eps);
}

__global__ __launch_bounds__(256) void bn_bwd_kernel(const float *X, int64_t ldx, const float *Y, int64_t ldy, const float *dY, int64_t ldd,
                                                      int64_t n_rows, int32_t n_feat, const float *mean, const float *rstd,
                                                      const float *gamma, const float *dbeta, const float *dgamma, int relu, float *dX,
                                                      int64_t ldo, const float *var, const float *beta, float eps, float inv_n,
                                                      int quirk)
{
    int64_t total = n_rows * n_feat;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t r = i / n_feat;
        int32_t f = (int32_t)(i - r * n_feat);
        float g = dY[r * ldd + f];
        const float x = X[r * ldx + f];
        if (relu && !relu_passed(Y, r * ldy + f, x, f, mean, var, eps, gamma, beta)) g = 0.f;
        if (mean && quirk) {
            // what reaches the transform in the REFERENCE: only the first arrival at BatchNorm's input, the direct path
            // Mul::_backward (g * gammas, operation.h:159-164) -> Div::_backward (/ (var + eps)^0.5, operation.h:192-198); the
            // arrivals through mean and var find the transform's op already done and are dropped (operation.h:80-88)
            if (gamma) g = __fmul_rn(g, gamma[f]);
            g = __fdiv_rn(g, sqrtf(__fadd_rn(var[f], eps)));
        } else if (mean) {
            float xhat = (x - mean[f]) * rstd[f];
            float gm = gamma ? gamma[f] : 1.f;
            g = gm * rstd[f] * (g - dbeta[f] * inv_n - xhat * dgamma[f] * inv_n);
        }
        dX[r * ldo + f] = g;
    }
}

// ---- 16 bytes per lane forms of the two backward passes (widths that are multiples of 4 up to 1024) ---------------------------
// Thread -> (row slot rr, quad of columns cq); the column constants (mean, 1/sigma, sigma, gamma, beta and, for the apply pass, the
// scaled sums) live in registers, four rows per thread are in flight.  The element arithmetic is the scalar kernels' (the ReLU
// decision without a stored forward output redoes the forward's sub / div / mul / add on x, each separately rounded); only the
// ORDER of the column sums differs (rows of a slot in order, slots in order, blocks in order: fixed, deterministic).
struct BnBwdVecArgs {
    const float *X, *Y, *dY, *mean, *var, *gamma, *beta;
    int64_t ldx, ldy, ldd, n_rows, rows_per_block;
    int32_t n_feat;
    int relu, quirk;
    float eps, inv_n;
    float *partial0, *partial1;        // MODE 0: [blocks][n_feat] sums of g and of g * xhat
    const float *dbeta, *dgamma;       // MODE 1
    float *dX;
    int64_t ldo;
};

template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_vec_kernel(BnBwdVecArgs p)
{
    __shared__ float red[MODE == 0 ? 2 * 256 * 4 : 1];
    const int q = p.n_feat >> 2, rpp = 256 / q;
    const int cq = threadIdx.x % q, rr = threadIdx.x / q;
    const bool live = rr < rpp;
    const int32_t f = 4 * cq;
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4] = {1.f, 1.f, 1.f, 1.f}, sd[4] = {1.f, 1.f, 1.f, 1.f}, gm[4] = {1.f, 1.f, 1.f, 1.f},
          bt[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f}, dg[4] = {0.f, 0.f, 0.f, 0.f};
    double rsd[4] = {1.0, 1.0, 1.0, 1.0};   // RN_f64(1 / sd): the forward's division as one f64 multiply (gnnx_common.h: div_by_const)
    const bool stats = p.mean != nullptr;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (stats) {
            mean[c] = p.mean[f + c];
            sd[c] = sqrtf(__fadd_rn(p.var[f + c], p.eps));      // (var + eps)->pow(0.5), the forward's divisor
            rsd[c] = 1.0 / (double)sd[c];
            rstd[c] = 1.0f / sqrtf(p.var[f + c] + p.eps);
            if (p.gamma) gm[c] = p.gamma[f + c];
            if (p.beta) bt[c] = p.beta[f + c];
            if (MODE == 1 && !p.quirk) {
                db[c] = p.dbeta[f + c] * p.inv_n;
                dg[c] = p.dgamma[f + c];
            }
        }
    }
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int64_t r1 = r0 + p.rows_per_block < p.n_rows ? r0 + p.rows_per_block : p.n_rows;
    if (live) {
        for (int64_t rb = r0 + rr; rb < r1; rb += 4 * (int64_t)rpp) {
            float4 x[4], g[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t r = rb + u * (int64_t)rpp;
                if (r < r1) {
                    x[u] = *reinterpret_cast<const float4 *>(p.X + r * p.ldx + f);
                    g[u] = *reinterpret_cast<const float4 *>(p.dY + r * p.ldd + f);
                    if (p.relu && p.Y) y[u] = *reinterpret_cast<const float4 *>(p.Y + r * p.ldy + f);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t r = rb + u * (int64_t)rpp;
                if (r >= r1) break;
                const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
                float gs[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
                const float ys[4] = {y[u].x, y[u].y, y[u].z, y[u].w};
                float o[4];
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if (p.relu) {
                        bool pass;
                        if (p.Y) pass = ys[c] > 0.f;
                        else {
                            float v = xs[c];
                            if (stats) {
                                v = div_by_const(__fsub_rn(v, mean[c]), sd[c], rsd[c]);
                                if (p.gamma) v = __fmul_rn(v, gm[c]);
                                if (p.beta) v = __fadd_rn(v, bt[c]);
                            }
                            pass = v > 0.f;
                        }
                        if (!pass) gs[c] = 0.f;
                    }
                    if (MODE == 0) {
                        const float xhat = (xs[c] - mean[c]) * rstd[c];
                        a0[c] += gs[c];
                        a1[c] += gs[c] * xhat;
                    } else {
                        float v = gs[c];
                        if (stats && p.quirk) {
                            if (p.gamma) v = __fmul_rn(v, gm[c]);
                            v = __fdiv_rn(v, sd[c]);
                        } else if (stats) {
                            const float xhat = (xs[c] - mean[c]) * rstd[c];
                            v = gm[c] * rstd[c] * (v - db[c] - xhat * dg[c] * p.inv_n);   // the scalar kernel's association
                        }
                        o[c] = v;
                    }
                }
                if (MODE == 1) *reinterpret_cast<float4 *>(p.dX + r * p.ldo + f) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    if (MODE == 0) {
        float4 *r0v = reinterpret_cast<float4 *>(red), *r1v = r0v + 256;
        r0v[threadIdx.x] = make_float4(a0[0], a0[1], a0[2], a0[3]);
        r1v[threadIdx.x] = make_float4(a1[0], a1[1], a1[2], a1[3]);
        __syncthreads();
        if (rr == 0) {
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
            for (int k = 0; k < rpp; k++) {
                const float4 u0 = r0v[k * q + cq], u1 = r1v[k * q + cq];
                s0.x += u0.x; s0.y += u0.y; s0.z += u0.z; s0.w += u0.w;
                s1.x += u1.x; s1.y += u1.y; s1.z += u1.z; s1.w += u1.w;
            }
            *reinterpret_cast<float4 *>(p.partial0 + (int64_t)blockIdx.x * p.n_feat + f) = s0;
            *reinterpret_cast<float4 *>(p.partial1 + (int64_t)blockIdx.x * p.n_feat + f) = s1;
        }
    }
}

// forward apply, 16 bytes per lane: the scalar kernel's arithmetic (sub, div by (var + eps)^0.5, mul, add, each rounded) with the
// column constants in registers and four rows per thread in flight
__global__ __launch_bounds__(256) void bn_fwd_vec_kernel(const float *X, int64_t ldx, int64_t n_rows, int32_t n_feat, const float *mean,
                                                          const float *var, float eps, const float *gamma, const float *beta, int relu,
                                                          float *Y, int64_t ldy, int64_t rows_per_block)
{
    const int q = n_feat >> 2, rpp = 256 / q;
    const int cq = threadIdx.x % q, rr = threadIdx.x / q;
    if (rr >= rpp) return;
    const int32_t f = 4 * cq;
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, sd[4] = {1.f, 1.f, 1.f, 1.f}, gm[4] = {1.f, 1.f, 1.f, 1.f}, bt[4] = {0.f, 0.f, 0.f, 0.f};
    double rsd[4] = {1.0, 1.0, 1.0, 1.0};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (mean) {
            mu[c] = mean[f + c];
            sd[c] = sqrtf(__fadd_rn(var[f + c], eps));
            rsd[c] = 1.0 / (double)sd[c];
            if (gamma) gm[c] = gamma[f + c];
            if (beta) bt[c] = beta[f + c];
        }
    }
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    for (int64_t rb = r0 + rr; rb < r1; rb += 4 * (int64_t)rpp) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (rb + u * (int64_t)rpp < r1) x[u] = *reinterpret_cast<const float4 *>(X + (rb + u * (int64_t)rpp) * ldx + f);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t r = rb + u * (int64_t)rpp;
            if (r >= r1) break;
            float v[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (mean) {
                    v[c] = div_by_const(__fsub_rn(v[c], mu[c]), sd[c], rsd[c]);   // == __fdiv_rn: one f64 multiply (gnnx_common.h)
                    if (gamma) v[c] = __fmul_rn(v[c], gm[c]);
                    if (beta) v[c] = __fadd_rn(v[c], bt[c]);
                }
                if (relu) v[c] = v[c] > 0.f ? v[c] : 0.f;
            }
            *reinterpret_cast<float4 *>(Y + r * ldy + f) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

inline bool bn_vec_ok(int32_t n_feat, const void *a, int64_t lda, const void *b, int64_t ldb, const void *c, int64_t ldc, const void *d,
                      int64_t ldd)
{
    auto al = [](const void *ptr, int64_t ld) { return !ptr || ((reinterpret_cast<uintptr_t>(ptr) & 15u) == 0 && ld % 4 == 0); };
    return n_feat % 4 == 0 && n_feat <= 1024 && al(a, lda) && al(b, ldb) && al(c, ldc) && al(d, ldd);
}

int64_t apply_block_cap()
{
    static const int cap_env = [] { const char *e = experiment_env("GNNX_BN_APPLY_BLOCKS"); return e ? atoi(e) : 0; }();   // A/B
    return cap_env > 0 ? cap_env : 8192;
}

int pick_fw(int32_t n_feat)
{
    int fw = 1;
    while (fw < n_feat && fw < 256) fw <<= 1;
    return fw;
}
int n_blocks_for(int64_t n_rows)
{
    int64_t b = ceil_div(n_rows, 64);
    static const int cap_env = [] { const char *e = experiment_env("GNNX_BN_REDUCE_BLOCKS"); return e ? atoi(e) : 0; }();   // A/B
    const int64_t cap = cap_env > 0 ? cap_env : kBlocks;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <class OP>
int reduce(OP op, int64_t n_rows, int32_t n_feat, float scale, float *out0, float *out1, float *ws, hipStream_t st)
{
    int nb = n_blocks_for(n_rows);
    int64_t rpb = ceil_div(n_rows > 0 ? n_rows : 1, nb);
    float *p0 = ws, *p1 = ws + (size_t)nb * n_feat;
    hipLaunchKernelGGL(colreduce_stage1<OP>, dim3(nb), dim3(256), 0, st, op, n_rows, n_feat, pick_fw(n_feat), rpb, p0, p1);
    GNNX_LAUNCH_CHECK();
    dim3 g2((uint32_t)ceil_div(n_feat, 64));
    hipLaunchKernelGGL(colreduce_stage2, g2, dim3(256), 0, st, p0, nb, n_feat, scale, out0);
    GNNX_LAUNCH_CHECK();
    if (OP::kTwo) {
        hipLaunchKernelGGL(colreduce_stage2, g2, dim3(256), 0, st, p1, nb, n_feat, scale, out1);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

int launch_bn_apply_vec(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd, int64_t n_rows,
                        int32_t n_feat, const float *d_mean, const float *d_var, float eps, const float *d_gamma, const float *d_beta, int relu,
                        const float *d_dgamma, const float *d_dbeta, float inv_n, int quirk, float *d_dX, int64_t ldo, hipStream_t st)
{
    const int rows_pass = 4 * (256 / (n_feat / 4));   // rows one workgroup has in flight
    int64_t nb = ceil_div(n_rows, (int64_t)rows_pass);
    if (nb > apply_block_cap()) nb = apply_block_cap();
    BnBwdVecArgs p{};
    p.X = d_X; p.Y = d_Y; p.dY = d_dY; p.mean = d_mean; p.var = d_var; p.gamma = d_gamma; p.beta = d_beta;
    p.ldx = ldx; p.ldy = ldy; p.ldd = ldd; p.n_rows = n_rows; p.rows_per_block = ceil_div(n_rows, nb); p.n_feat = n_feat;
    p.relu = relu; p.quirk = quirk; p.eps = eps; p.inv_n = inv_n; p.dbeta = d_dbeta; p.dgamma = d_dgamma; p.dX = d_dX; p.ldo = ldo;
    hipLaunchKernelGGL(bn_bwd_vec_kernel<1>, dim3((uint32_t)nb), dim3(256), 0, st, p);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_bn_workspace(int64_t n_rows, int32_t n_feat, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_rows >= 0 && n_feat >= 0, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = sizeof(float) * ((size_t)2 * n_blocks_for(n_rows) + 1) * (size_t)(n_feat > 0 ? n_feat : 1);
    return GNNX_OK;
}

GNNX_API int gnnx_bn_stats_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, float *d_mean, float *d_var,
                               void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_rows > 0 && n_feat > 0, GNNX_ERR_INVALID_ARG, "empty batch");
    GNNX_REQUIRE(d_X && d_mean && d_var && ldx >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld < n_feat");
    size_t need = 0;
    gnnx_bn_workspace(n_rows, n_feat, &need);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(d_workspace);
    const float inv_n = 1.0f / (float)n_rows;
    int rc = reduce(OpIdent{d_X, ldx}, n_rows, n_feat, inv_n, d_mean, nullptr, ws, st);
    if (rc) return rc;
    return reduce(OpSqDev{d_X, ldx, d_mean}, n_rows, n_feat, inv_n, d_var, nullptr, ws, st);
}

GNNX_API int gnnx_bn_relu_fwd_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, const float *d_mean,
                                  const float *d_var, float eps, const float *d_gamma, const float *d_beta, int relu, float *d_Y,
                                  int64_t ldy, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_feat >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    if (n_rows == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(d_X && d_Y && ldx >= n_feat && ldy >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld < n_feat");
    GNNX_REQUIRE((d_mean == nullptr) == (d_var == nullptr), GNNX_ERR_INVALID_ARG, "mean and var go together");
    if (bn_vec_ok(n_feat, d_X, ldx, d_Y, ldy, nullptr, 0, nullptr, 0)) {
        const int rows_pass = 4 * (256 / (n_feat / 4));
        int64_t nb = ceil_div(n_rows, (int64_t)rows_pass);
        if (nb > apply_block_cap()) nb = apply_block_cap();
        hipLaunchKernelGGL(bn_fwd_vec_kernel, dim3((uint32_t)nb), dim3(256), 0, as_stream(stream), d_X, ldx, n_rows, n_feat, d_mean, d_var, eps,
                           d_gamma, d_beta, relu, d_Y, ldy, ceil_div(n_rows, nb));
        GNNX_LAUNCH_CHECK();
        return GNNX_OK;
    }
    int64_t blocks = ceil_div(n_rows * n_feat, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bn_fwd_kernel, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), d_X, ldx, n_rows, n_feat, d_mean, d_var,
                       eps, d_gamma, d_beta, relu, d_Y, ldy);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

// cross-shard form of the statistics: out[f] = scale * sum_i x_if (d_mean == NULL) or scale * sum_i (x_if - mean_f)^2; a sharded
// BatchNorm all-reduces these [F] vectors with scale = 1 / N_global (mean first, then the centred squares against the GLOBAL mean:
// the same exact two-pass variance as gnnx_bn_stats_f32)
GNNX_API int gnnx_bn_partial_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, const float *d_mean, float scale,
                                 float *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_feat > 0, GNNX_ERR_INVALID_ARG, "bad sizes");
    GNNX_REQUIRE(d_out && (n_rows == 0 || d_X) && ldx >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld < n_feat");
    size_t need = 0;
    gnnx_bn_workspace(n_rows, n_feat, &need);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(d_workspace);
    if (d_mean) return reduce(OpSqDev{d_X, ldx, d_mean}, n_rows, n_feat, scale, d_out, nullptr, ws, st);
    return reduce(OpIdent{d_X, ldx}, n_rows, n_feat, scale, d_out, nullptr, ws, st);
}

static int bn_bwd_check(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd, int64_t n_rows,
                        int32_t n_feat, const float *d_mean, const float *d_var, void *d_workspace, size_t workspace_bytes)
{
    GNNX_REQUIRE(n_rows > 0 && n_feat > 0, GNNX_ERR_INVALID_ARG, "empty batch");
    GNNX_REQUIRE(d_X && d_dY && ldx >= n_feat && ldd >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld");
    GNNX_REQUIRE(!d_Y || ldy >= n_feat, GNNX_ERR_INVALID_ARG, "ldy < n_feat");
    GNNX_REQUIRE((d_mean == nullptr) == (d_var == nullptr), GNNX_ERR_INVALID_ARG, "mean and var go together");
    if (d_mean) {
        size_t need = 0;
        gnnx_bn_workspace(n_rows, n_feat, &need);
        GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    }
    return GNNX_OK;
}

// the two halves of gnnx_bn_relu_bwd_f32, separable so that a sharded BatchNorm can all-reduce dgamma / dbeta in between:
//   sums : d_dbeta = sum_i g_i, d_dgamma = sum_i g_i * xhat_i over THIS call's rows
//   apply: dX = gamma / sigma * (g - dbeta / n_total - xhat * dgamma / n_total) with the (global) sums and row count handed in
GNNX_API int gnnx_bn_relu_bwd_sums_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                                       int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps,
                                       const float *d_gamma, const float *d_beta, int relu, float *d_dgamma, float *d_dbeta,
                                       void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = bn_bwd_check(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, d_workspace, workspace_bytes);
    if (rc) return rc;
    GNNX_REQUIRE(d_mean && d_dgamma && d_dbeta, GNNX_ERR_INVALID_ARG, "statistics and dgamma / dbeta outputs are required");
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(d_workspace);
    float *rstd = ws + (size_t)2 * n_blocks_for(n_rows) * n_feat;
    if (bn_vec_ok(n_feat, d_X, ldx, d_Y, ldy, d_dY, ldd, ws, 4)) {
        const int nb = n_blocks_for(n_rows);
        BnBwdVecArgs p{};
        p.X = d_X; p.Y = d_Y; p.dY = d_dY; p.mean = d_mean; p.var = d_var; p.gamma = d_gamma; p.beta = d_beta;
        p.ldx = ldx; p.ldy = ldy; p.ldd = ldd; p.n_rows = n_rows; p.rows_per_block = ceil_div(n_rows, nb); p.n_feat = n_feat;
        p.relu = relu; p.eps = eps; p.partial0 = ws; p.partial1 = ws + (size_t)nb * n_feat;
        hipLaunchKernelGGL(bn_bwd_vec_kernel<0>, dim3(nb), dim3(256), 0, st, p);
        GNNX_LAUNCH_CHECK();
        dim3 g2((uint32_t)ceil_div(n_feat, 64));
        hipLaunchKernelGGL(colreduce_stage2, g2, dim3(256), 0, st, p.partial0, nb, n_feat, 1.0f, d_dbeta);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(colreduce_stage2, g2, dim3(256), 0, st, p.partial1, nb, n_feat, 1.0f, d_dgamma);
        GNNX_LAUNCH_CHECK();
        return GNNX_OK;
    }
    hipLaunchKernelGGL(rstd_kernel, dim3((uint32_t)ceil_div(n_feat, 256)), dim3(256), 0, st, d_var, eps, n_feat, rstd);
    GNNX_LAUNCH_CHECK();
    return reduce(OpBnBwd{d_X, d_Y, d_dY, d_mean, rstd, ldx, ldy, ldd, relu, d_var, d_gamma, d_beta, eps}, n_rows, n_feat, 1.0f, d_dbeta,
                  d_dgamma, ws, st);
}

GNNX_API int gnnx_bn_relu_bwd_apply_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                                        int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps,
                                        const float *d_gamma, const float *d_beta, int relu, const float *d_dgamma, const float *d_dbeta,
                                        int64_t n_total, float *d_dX, int64_t ldo, void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = bn_bwd_check(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, d_workspace, workspace_bytes);
    if (rc) return rc;
    GNNX_REQUIRE(d_dX && ldo >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld");
    GNNX_REQUIRE(!d_mean || (d_dgamma && d_dbeta && n_total >= n_rows), GNNX_ERR_INVALID_ARG, "dgamma / dbeta sums and n_total are required");
    hipStream_t st = as_stream(stream);
    if (bn_vec_ok(n_feat, d_X, ldx, d_Y, ldy, d_dY, ldd, d_dX, ldo)) return launch_bn_apply_vec(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat,
            d_mean, d_var, eps, d_gamma, d_beta, relu, d_dgamma, d_dbeta, d_mean ? 1.0f / (float)n_total : 0.f, 0, d_dX, ldo, st);
    int64_t blocks = ceil_div(n_rows * n_feat, 256);
    if (blocks > 4096) blocks = 4096;
    const float *rstd = nullptr;
    if (d_mean) {
        float *ws = static_cast<float *>(d_workspace);
        float *r = ws + (size_t)2 * n_blocks_for(n_rows) * n_feat;
        hipLaunchKernelGGL(rstd_kernel, dim3((uint32_t)ceil_div(n_feat, 256)), dim3(256), 0, st, d_var, eps, n_feat, r);
        GNNX_LAUNCH_CHECK();
        rstd = r;
    }
    hipLaunchKernelGGL(bn_bwd_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, rstd,
                       d_gamma, d_dbeta, d_dgamma, relu, d_dX, ldo, d_var, d_beta, eps, d_mean ? 1.0f / (float)n_total : 0.f, 0);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

// OPT-IN "reference-quirk" backward: dgamma / dbeta as usual, but dX = (g * gamma) / (var + eps)^0.5 --
// the batch statistics treated as constants, which is what the reference's traversal delivers (see bn_bwd_kernel).  Only for
// comparing gradients with the reference's own; never the default.
GNNX_API int gnnx_bn_relu_bwd_quirk_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                                        int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps,
                                        const float *d_gamma, const float *d_beta, int relu, float *d_dX, int64_t ldo, float *d_dgamma,
                                        float *d_dbeta, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(d_mean && d_var, GNNX_ERR_INVALID_ARG, "the quirk form is about BatchNorm: statistics are required");
    // every refusal comes before the sums half writes dgamma / dbeta: a refused call leaves all outputs alone
    int rc = bn_bwd_check(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, d_workspace, workspace_bytes);
    if (rc) return rc;
    GNNX_REQUIRE(d_dX && ldo >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld");
    rc = gnnx_bn_relu_bwd_sums_f32(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, eps, d_gamma, d_beta, relu, d_dgamma,
                                       d_dbeta, d_workspace, workspace_bytes, stream);
    if (rc) return rc;
    if (bn_vec_ok(n_feat, d_X, ldx, d_Y, ldy, d_dY, ldd, d_dX, ldo))
        return launch_bn_apply_vec(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, eps, d_gamma, d_beta, relu, d_dgamma, d_dbeta,
                                   0.f, 1, d_dX, ldo, as_stream(stream));
    int64_t blocks = ceil_div(n_rows * n_feat, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bn_bwd_kernel, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat,
                       d_mean, (const float *)nullptr, d_gamma, (const float *)d_dbeta, (const float *)d_dgamma, relu, d_dX, ldo, d_var,
                       d_beta, eps, 0.f, 1);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_bn_relu_bwd_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                                  int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps,
                                  const float *d_gamma, const float *d_beta, int relu, float *d_dX, int64_t ldo, float *d_dgamma,
                                  float *d_dbeta, void *d_workspace, size_t workspace_bytes, void *stream)
{
    // the apply half's refusals first: the sums half writes dgamma / dbeta, and a refused call leaves all outputs alone
    int rc = bn_bwd_check(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, d_workspace, workspace_bytes);
    if (rc) return rc;
    GNNX_REQUIRE(d_dX && ldo >= n_feat, GNNX_ERR_INVALID_ARG, "null pointer or ld");
    if (d_mean) {
        rc = gnnx_bn_relu_bwd_sums_f32(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, eps, d_gamma, d_beta, relu, d_dgamma,
                                       d_dbeta, d_workspace, workspace_bytes, stream);
        if (rc) return rc;
    }
    return gnnx_bn_relu_bwd_apply_f32(d_X, ldx, d_Y, ldy, d_dY, ldd, n_rows, n_feat, d_mean, d_var, eps, d_gamma, d_beta, relu, d_dgamma,
                                      d_dbeta, n_rows, d_dX, ldo, d_workspace, workspace_bytes, stream);
}
