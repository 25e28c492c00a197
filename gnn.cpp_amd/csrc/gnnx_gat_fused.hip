// Graph attention (GATv1) without per-entry arrays: score, softmax and aggregation in one gather -- include/gnnx.h "fused graph
// attention".  The score of an entry is a function of two per-vertex scalars per head,
//   t_p = rowterm[i, h] + colterm[c_p, h];  e_p = leaky_relu(t_p);  m_i = max_p e_p;  x_p = expf(e_p - m_i);  z_i = sum_p x_p,
// so alpha_p = x_p / z_i is recomputed wherever it is needed from [n, H] arrays.  Three calls:
//   forward    Y[i, f]  = act( (sum_p x_p X[c_p, f]) / z_i + bias[f] ),  rowmax = m, rowsum = z
//   bwd, rows  dot[i, h] = <G_i, Y_i - bias>_h;  drowterm[i, h] = sum_p dt_p            (forward pattern)
//   bwd, cols  dX[c, f] (+)= sum_i alpha_ic G[i, f];  dcolterm[c, h] = sum_i dt_ic       (transposed pattern)
// with dalpha_p = <G_i, X_c>_h, de_p = alpha_p (dalpha_p - dot_i), dt_p = t_p > 0 ? de_p : de_p slope.  No transpose map, no [nnz, .]
// array, no atomic on a value.
//
// ORDER (the contract; a function of the row length and of D alone).  The maximum is taken first and is exact, so nothing is rescaled
// and partial sums combine by plain addition.  Every sum over a row's entries (z, the numerator, drowterm, dX, dcolterm) is ONE
// accumulator per output element over the entries of a segment of S = 4096 consecutive entries in ascending order from +0, and the
// segments' sums are added in ascending order starting from the first; a row of d <= S entries is one segment.  Every dot product over
// a head's D features (dot, dalpha) is the order of gnnx_edge_dot.h with F := D.  How rows, heads and features map to lanes is not in
// the result.
//
// LANES.  A head is a group of GH = min(64, pow2 >= ceil(D / 4)) lanes, lane lh owns the 16-byte chunks lh, lh + GH, ... of the head's
// slab (more than one only for D > 256; at most kMaxChunks, so D <= 512); a row is a group of GE = min(64, pow2 >= GH H) lanes that
// holds HP = GE / GH heads, further heads are further passes in grid.y (for D % 4 == 0 and H D <= 256 this is "lane l owns features
// 4 l .. 4 l + 3", the piece layout of gnnx_heads.hip; a head never straddles two workgroups, which the backward's dot products
// need).  The group loads GE column indices at once and hands them out by shuffle.  Each lane walks all the row's entries for its
// head: sweep 1 gathers only the column's scalar (lanes of one head read one address, an entry's H scalars are one sector) and every
// lane of a head ends with the same maximum, no shuffle; sweep 2 requests four gathered chunks and their scalars before the first
// expf.  One expf per lane and entry.
//   * e_p is recomputed in sweep 2 from a second scalar gather for every row length; keeping the e of a short row in registers
//     between the sweeps was not built (it needs a second copy of the sweep for rows of at most GE entries); not measured.
//   * chunks that are not 16-byte loadable (D % 4 != 0, a leading dimension or pointer off 16 bytes) are loaded by four guarded
//     scalar loads into the SAME chunk: one kernel source, same order, same bits -- instead of a one-float-per-lane layout, whose
//     dot products would need a second order.
// HUBS (d > S).  The row kernel lists them (gnnx_worklist.h) and leaves them alone; lane groups of a fixed grid then stride over the
// segment slots.  Forward: segment maxima -> a thread per (hub, head) takes their maximum -> a second segment pass writes (z_s,
// N_s[F]) per slot -> a thread per (hub, element) adds the slots ascending, divides and applies the epilogue.  The backward calls
// need one segment pass and the combine.  (The hub maximum is a thread per (hub, head), not a wavefront per hub: a hub has at most
// nnz / S segments and the launch is not on any measured path.)  All of it is skipped on the host when nnz <= S.
// GH (in the forward), GE and HP are run-time values: a lane pays an integer division and run-time masks once per row, and the
// entry loops run over a window whose size the compiler does not know.  Left so for one forward source per chunk count; what
// templates on GE would gain was not measured, and with the time a latency chain it is an open candidate.
// No matrix instruction fits: there is no dense operand reuse, the work is a gather with about 3 flops per gathered float.
#include "gnnx_edge_dot.h"
#include "gnnx_worklist.h"

#include <type_traits>

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kCounters = 16;      // int32 words in front of the workspace: [0], [1] the hub list's
constexpr int kSegGroups = 8192;   // lane groups of a segment pass (stride over the slots)
constexpr int kMaxChunks = 2;      // chunks per lane: D <= 4 * 64 * kMaxChunks

struct Work {
    int32_t *counters;
    HubList hubs;
    float *hub_max;   // [cap_hub, H] the forward's row maxima of the hubs
    float *part_h;    // [cap_seg, H] per slot and head: the segment's maximum, later its z_s (forward); its sum of dt (backward)
    float *part_f;    // [cap_seg, F] per slot and feature: N_s (forward), the dX partial (column side)
};

// The caller's pointer is aligned to 256 bytes and the counters take 64, so part_f is stored in 16-byte chunks.  cap_hub <= cap_seg, so
// the arrays fit the neighbourhood reductions' workspace (two arrays of cap_seg * width words) at width = F + H: take_workspace().
size_t carve(int32_t n_rows, int64_t nnz, int32_t H, int64_t F, void *base, Work *out)
{
    Work w{};
    w.hubs.size(n_rows, nnz);
    Carver c(base ? aligned_base(base) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);
    w.part_f = c.take<float>((size_t)w.hubs.cap_seg * F, 16);
    w.part_h = c.take<float>((size_t)w.hubs.cap_seg * H, 4);
    w.hub_max = c.take<float>((size_t)w.hubs.cap_hub * H, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hubs.take_slots(c);
    if (out) *out = w;
    return c.bytes();
}

// One struct for the three calls.  "own" is the row of the pattern the call runs on, "gathered" the entry's column.
struct Args {
    int32_t n_rows, H, D;
    const int32_t *rowptr, *colidx;
    const float *rowterm;   // forward, row side: own; column side: gathered
    int64_t rs;
    const float *colterm;   // forward, row side: gathered; column side: own
    int64_t cs;
    float slope;
    const float *X;         // forward, row side: gathered; column side: own
    int64_t ldx;
    const float *G;         // row side: own; column side: gathered
    int64_t ldg;
    const float *Yin;       // row side: the forward's output
    int64_t ldyin;
    const float *bias;
    const float *rowmax, *rowsum, *dot;        // backward inputs, [n, H] (dot: column side)
    float *rowmax_out, *rowsum_out, *dot_out;  // forward outputs; row side: dot
    float *Y;               // forward: Y; column side: dX
    int64_t ldy;
    int beta, relu_out;
    float *dterm;           // drowterm / dcolterm
    int64_t ds;
    int32_t GH, GE, HP;     // lanes per head, lanes per row, heads per pass
    Work w;
};

template <int N> using Int = std::integral_constant<int, N>;

__device__ __forceinline__ float leaky_of(float t, float slope) { return t > 0.f ? t : t * slope; }
__device__ __forceinline__ float4 mul_add(float4 acc, float4 x, float v)   // each product rounded, then the sum
{
    return make_float4(acc.x + (x.x * v), acc.y + (x.y * v), acc.z + (x.z * v), acc.w + (x.w * v));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

template <bool VEC>
__device__ __forceinline__ void store_chunk(float *p, const float4 &v, int32_t rem)
{
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(p) = v;
    } else {
        p[0] = v.x;
        if (rem > 1) p[1] = v.y;
        if (rem > 2) p[2] = v.z;
        if (rem > 3) p[3] = v.w;
    }
}

// where a lane stands: in its row's group, in its head's group, and which chunks it owns
struct Lane {
    int li, gbase, lh;
    int32_t h, hs, Q, D, GH;
    bool head_ok;
    __device__ __forceinline__ explicit Lane(const Args &a)
    {
        li = threadIdx.x & (a.GE - 1);
        gbase = (threadIdx.x & 63) - li;
        lh = li & (a.GH - 1);
        h = (int32_t)blockIdx.y * a.HP + li / a.GH;
        head_ok = h < a.H;
        hs = head_ok ? h : 0;   // lanes without a head read head 0's scalars and store nothing
        Q = (a.D + 3) >> 2;
        D = a.D;
        GH = a.GH;
    }
    __device__ __forceinline__ bool has(int j) const { return head_ok && lh + j * GH < Q; }
    __device__ __forceinline__ int64_t off(int j) const { return (int64_t)h * D + 4 * (int64_t)(lh + j * GH); }
    __device__ __forceinline__ int32_t rem(int j) const { return D - 4 * (lh + j * GH); }   // features of the head from the chunk on
    __device__ __forceinline__ bool first() const { return head_ok && lh == 0; }            // the lane that stores the head's scalars
};

// the lane group that runs the row (row kernels) or strides over the segment slots (segment kernels)
__device__ __forceinline__ int64_t group_index(const Args &a) { return ((int64_t)blockIdx.x * 256 + threadIdx.x) / a.GE; }
__device__ __forceinline__ int64_t group_count(const Args &a) { return (int64_t)gridDim.x * 256 / a.GE; }

// body(Int<B>, c[B]) for the entries b .. b + n - 1 in ascending order, four at a time while four are left in the window of GE
// indices that the group loaded at once.  Every lane of the group passes the same (b, n): the body may shuffle inside the group.
template <class Body>
__device__ __forceinline__ void for_entries(const Args &a, const Lane &ln, int64_t b, int64_t n, Body body)
{
    for (int64_t w0 = 0; w0 < n; w0 += a.GE) {
        const int64_t q = w0 + ln.li;
        const int32_t myc = a.colidx[b + (q < n ? q : n - 1)];
        const int cnt = n - w0 < a.GE ? (int)(n - w0) : a.GE;
        int k = 0;
        for (; k + 4 <= cnt; k += 4) {
            int32_t c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) c[u] = __shfl(myc, ln.gbase + k + u, 64);
            body(Int<4>{}, c);
        }
        for (; k < cnt; k++) {
            int32_t c[1] = {__shfl(myc, ln.gbase + k, 64)};
            body(Int<1>{}, c);
        }
    }
}

// sweep 1: the maximum of e_p over the entries, for the lane's head; own = the own row's term, `gathered` the other term's array
__device__ __forceinline__ float sweep_max(const Args &a, const Lane &ln, int64_t b, int64_t n, float own, const float *gathered, int64_t gs)
{
    float m = -INFINITY;
    for_entries(a, ln, b, n, [&](auto bt, const int32_t *c) {
        constexpr int B = decltype(bt)::value;
        float t[B];
#pragma unroll
        for (int u = 0; u < B; u++) t[u] = gathered[(int64_t)c[u] * gs + ln.hs];
#pragma unroll
        for (int u = 0; u < B; u++) m = fmaxf(m, leaky_of(own + t[u], a.slope));
    });
    return m;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
// sweep 2 over the entries b .. b + n - 1: z += x_p, acc[j] += x_p * X[c_p, chunk j]
template <int CH, bool VEC>
__device__ __forceinline__ void fwd_entries(const Args &a, const Lane &ln, int64_t b, int64_t n, float rt, float m, float &z, float4 (&acc)[CH])
{
    for_entries(a, ln, b, n, [&](auto bt, const int32_t *c) {
        constexpr int B = decltype(bt)::value;
        float ct[B];
        float4 x[B][CH];
#pragma unroll
        for (int u = 0; u < B; u++) {
            ct[u] = a.colterm[(int64_t)c[u] * a.cs + ln.hs];
#pragma unroll
            for (int j = 0; j < CH; j++)
                x[u][j] = ln.has(j) ? load_chunk<VEC>(a.X + (int64_t)c[u] * a.ldx + ln.off(j), 0, ln.rem(j)) : zero4();
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            const float xv = expf(leaky_of(rt + ct[u], a.slope) - m);
            z = z + xv;
#pragma unroll
            for (int j = 0; j < CH; j++) acc[j] = mul_add(acc[j], x[u][j], xv);
        }
    });
}

// (N / z, or +0 for an empty row) + bias, ReLU
template <bool VEC>
__device__ __forceinline__ float4 fwd_epilogue(const Args &a, const Lane &ln, int j, float4 N, float z, bool empty)
{
    float4 y = empty ? zero4() : make_float4(__fdiv_rn(N.x, z), __fdiv_rn(N.y, z), __fdiv_rn(N.z, z), __fdiv_rn(N.w, z));
    if (a.bias) y = add4(y, load_chunk<VEC>(a.bias + ln.off(j), 0, ln.rem(j)));
    if (a.relu_out) y = make_float4(y.x > 0.f ? y.x : 0.f, y.y > 0.f ? y.y : 0.f, y.z > 0.f ? y.z : 0.f, y.w > 0.f ? y.w : 0.f);
    return y;
}

// grid.x: blocks of 256 / GE rows; grid.y: passes of HP heads
template <int CH, bool VEC>
__global__ __launch_bounds__(256) void fwd_rows_kernel(Args a)
{
    const Lane ln(a);
    const int64_t row = group_index(a);
    if (row >= a.n_rows) return;   // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int64_t b = a.rowptr[row];
    int64_t d = (int64_t)a.rowptr[row + 1] - b;
    d = d < 0 ? 0 : d;
    if (d > kSeg) {
        if (blockIdx.y == 0 && ln.li == 0 && a.w.hubs.cap_hub > 0) append(a.w.hubs, (int32_t)row, d);
        return;
    }
    const float rt = a.rowterm[row * a.rs + ln.hs];
    const float m = sweep_max(a, ln, b, d, rt, a.colterm, a.cs);
    float z = 0.f;
    float4 acc[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) acc[j] = zero4();
    fwd_entries<CH, VEC>(a, ln, b, d, rt, m, z, acc);
#pragma unroll
    for (int j = 0; j < CH; j++)
        if (ln.has(j)) store_chunk<VEC>(a.Y + row * a.ldy + ln.off(j), fwd_epilogue<VEC>(a, ln, j, acc[j], z, d == 0), ln.rem(j));
    if (ln.first()) {
        if (a.rowmax_out) a.rowmax_out[row * a.H + ln.h] = m;   // an empty row: -inf
        if (a.rowsum_out) a.rowsum_out[row * a.H + ln.h] = z;   //               +0
    }
}

// the segments' maxima -> part_h
__global__ __launch_bounds__(256) void fwd_seg_max_kernel(Args a)
{
    const Lane ln(a);
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        const float m = sweep_max(a, ln, b, n, a.rowterm[(int64_t)row * a.rs + ln.hs], a.colterm, a.cs);
        if (ln.first()) a.w.part_h[slot * a.H + ln.h] = m;
    });
}

// a thread per (hub, head): the maximum of the segments' maxima -> hub_max, rowmax
__global__ __launch_bounds__(256) void hub_max_kernel(Args a)
{
    const int64_t total = listed_hubs(a.w.hubs) * a.H;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t hub = idx / a.H;
        const int32_t h = (int32_t)(idx - hub * a.H);
        const int32_t row = a.w.hubs.hub_rows[hub];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const float *part = a.w.part_h + (int64_t)a.w.hubs.hub_seg0[hub] * a.H + h;
        float m = -INFINITY;
        for (int64_t s = 0; s < nseg; s++) m = fmaxf(m, part[s * a.H]);
        a.w.hub_max[idx] = m;
        if (a.rowmax_out) a.rowmax_out[(int64_t)row * a.H + h] = m;
    }
}

// (z_s, N_s) of every segment -> part_h, part_f
template <int CH, bool VEC>
__global__ __launch_bounds__(256) void fwd_seg_acc_kernel(Args a)
{
    const Lane ln(a);
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t hub, int64_t, int64_t b, int64_t n, int64_t slot) {
        const float m = a.w.hub_max[(int64_t)hub * a.H + ln.hs];
        float z = 0.f;
        float4 acc[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) acc[j] = zero4();
        fwd_entries<CH, VEC>(a, ln, b, n, a.rowterm[(int64_t)row * a.rs + ln.hs], m, z, acc);
#pragma unroll
        for (int j = 0; j < CH; j++)
            if (ln.has(j)) store_chunk<VEC>(a.w.part_f + slot * ((int64_t)a.H * a.D) + ln.off(j), acc[j], ln.rem(j));
        if (ln.first()) a.w.part_h[slot * a.H + ln.h] = z;
    });
}

// A thread per (hub, element): the slots' partial sums added ascending from the first, then the call's epilogue.
//   MODE 0 (forward): Y = act(N / z + bias), rowsum = z;  MODE 1 (column side): dX (+)= N, dcolterm = the head's sum;
//   MODE 2 (row side): a thread per (hub, head), drowterm = the head's sum
template <int MODE>
__global__ __launch_bounds__(256) void hub_combine_kernel(Args a)
{
    const int64_t width = MODE == 2 ? a.H : (int64_t)a.H * a.D;
    const int64_t total = listed_hubs(a.w.hubs) * width;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t hub = idx / width;
        const int64_t f = idx - hub * width;
        const int32_t h = MODE == 2 ? (int32_t)f : (int32_t)(f / a.D);
        const int32_t row = a.w.hubs.hub_rows[hub];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t s0 = a.w.hubs.hub_seg0[hub];
        const float *ph = a.w.part_h + s0 * a.H + h;
        float sh = ph[0];
        for (int64_t s = 1; s < nseg; s++) sh = sh + ph[s * a.H];
        if constexpr (MODE == 2) {
            a.dterm[(int64_t)row * a.ds + h] = sh;
        } else {
            const float *pf = a.w.part_f + s0 * width + f;
            float N = pf[0];
            for (int64_t s = 1; s < nseg; s++) N = N + pf[s * width];
            float *dst = a.Y + (int64_t)row * a.ldy + f;
            if constexpr (MODE == 0) {
                float y = __fdiv_rn(N, sh);
                if (a.bias) y = y + a.bias[f];
                if (a.relu_out) y = y > 0.f ? y : 0.f;
                *dst = y;
                if (f == (int64_t)h * a.D && a.rowsum_out) a.rowsum_out[(int64_t)row * a.H + h] = sh;
            } else {
                *dst = a.beta ? *dst + N : N;
                if (f == (int64_t)h * a.D) a.dterm[(int64_t)row * a.ds + h] = sh;
            }
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// dt_p of one entry: alpha_p = x_p / z, de_p = alpha_p (dalpha_p - dot), through the leaky ReLU
__device__ __forceinline__ float dt_of(float t, float slope, float al, float da, float dot)
{
    const float de = al * (da - dot);
    return t > 0.f ? de : de * slope;
}

// <l, r> over the head's features in the order of gnnx_edge_dot.h with F := D: the lane's chunks ascending into one accumulator, then
// the butterfly over the head's GH lanes -- every lane of the head ends with the same bits
template <int GH, int CH, bool VEC>
__device__ __forceinline__ float head_dot(const Lane &ln, const float4 (&l)[CH], const float4 (&r)[CH])
{
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < CH; j++)
        if (ln.has(j)) acc = add_chunk<VEC>(acc, l[j], r[j], 0, ln.rem(j));
    return butterfly<GH>(acc);
}

// row side: the sum of dt_p over the entries b .. b + n - 1 of row i, whose G chunks are g[]
template <int GH, int CH, bool VEC>
__device__ __forceinline__ float rows_entries(const Args &a, const Lane &ln, int64_t b, int64_t n, const float4 (&g)[CH], float rt, float m, float z,
                                              float dot)
{
    float sum = 0.f;
    for_entries(a, ln, b, n, [&](auto bt, const int32_t *c) {
        constexpr int B = decltype(bt)::value;
        float ct[B];
        float4 x[B][CH];
#pragma unroll
        for (int u = 0; u < B; u++) {
            ct[u] = a.colterm[(int64_t)c[u] * a.cs + ln.hs];
#pragma unroll
            for (int j = 0; j < CH; j++)
                x[u][j] = ln.has(j) ? load_chunk<VEC>(a.X + (int64_t)c[u] * a.ldx + ln.off(j), 0, ln.rem(j)) : zero4();
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            const float t = rt + ct[u];
            const float al = __fdiv_rn(expf(leaky_of(t, a.slope) - m), z);
            sum = sum + dt_of(t, a.slope, al, head_dot<GH, CH, VEC>(ln, g, x[u]), dot);
        }
    });
    return sum;
}

template <int CH, bool VEC>
__device__ __forceinline__ void load_own(const Lane &ln, const float *rowp, float4 (&v)[CH])
{
#pragma unroll
    for (int j = 0; j < CH; j++) v[j] = ln.has(j) ? load_chunk<VEC>(rowp + ln.off(j), 0, ln.rem(j)) : zero4();
}

template <int GH, int CH, bool VEC>
__global__ __launch_bounds__(256) void bwd_rows_kernel(Args a)
{
    const Lane ln(a);
    const int64_t row = group_index(a);
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row];
    int64_t d = (int64_t)a.rowptr[row + 1] - b;
    d = d < 0 ? 0 : d;
    float4 g[CH], y[CH];
    load_own<CH, VEC>(ln, a.G + row * a.ldg, g);
    load_own<CH, VEC>(ln, a.Yin + row * a.ldyin, y);
    if (a.bias) {
#pragma unroll
        for (int j = 0; j < CH; j++)
            if (ln.has(j)) y[j] = sub4(y[j], load_chunk<VEC>(a.bias + ln.off(j), 0, ln.rem(j)));
    }
    const float dot = head_dot<GH, CH, VEC>(ln, g, y);
    if (ln.first()) a.dot_out[row * a.H + ln.h] = dot;
    if (d > kSeg) {   // the segment kernel reads dot back
        if (blockIdx.y == 0 && ln.li == 0 && a.w.hubs.cap_hub > 0) append(a.w.hubs, (int32_t)row, d);
        return;
    }
    const float sum = rows_entries<GH, CH, VEC>(a, ln, b, d, g, a.rowterm[row * a.rs + ln.hs], a.rowmax[row * a.H + ln.hs],
                                                a.rowsum[row * a.H + ln.hs], dot);
    if (ln.first()) a.dterm[row * a.ds + ln.h] = sum;   // an empty row: +0
}

template <int GH, int CH, bool VEC>
__global__ __launch_bounds__(256) void bwd_rows_seg_kernel(Args a)
{
    const Lane ln(a);
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        float4 g[CH];
        load_own<CH, VEC>(ln, a.G + (int64_t)row * a.ldg, g);
        const int64_t at = (int64_t)row * a.H + ln.hs;
        const float sum = rows_entries<GH, CH, VEC>(a, ln, b, n, g, a.rowterm[(int64_t)row * a.rs + ln.hs], a.rowmax[at], a.rowsum[at], a.dot_out[at]);
        if (ln.first()) a.w.part_h[slot * a.H + ln.h] = sum;
    });
}

// column side, on the transposed pattern: row c with X chunks xo[] and its own colterm ct; the entries are the rows i of the forward.
// acc[j] += alpha_ic * G[i, chunk j];  sum += dt_ic
template <int GH, int CH, bool VEC>
__device__ __forceinline__ void cols_entries(const Args &a, const Lane &ln, int64_t b, int64_t n, const float4 (&xo)[CH], float ct, float &sum,
                                             float4 (&acc)[CH])
{
    for_entries(a, ln, b, n, [&](auto bt, const int32_t *c) {
        constexpr int B = decltype(bt)::value;
        float rt[B], m[B], z[B], dot[B];
        float4 g[B][CH];
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int64_t at = (int64_t)c[u] * a.H + ln.hs;
            rt[u] = a.rowterm[(int64_t)c[u] * a.rs + ln.hs];
            m[u] = a.rowmax[at];
            z[u] = a.rowsum[at];
            dot[u] = a.dot[at];
#pragma unroll
            for (int j = 0; j < CH; j++)
                g[u][j] = ln.has(j) ? load_chunk<VEC>(a.G + (int64_t)c[u] * a.ldg + ln.off(j), 0, ln.rem(j)) : zero4();
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            const float t = rt[u] + ct;
            const float al = __fdiv_rn(expf(leaky_of(t, a.slope) - m[u]), z[u]);
            sum = sum + dt_of(t, a.slope, al, head_dot<GH, CH, VEC>(ln, g[u], xo), dot[u]);
#pragma unroll
            for (int j = 0; j < CH; j++) acc[j] = mul_add(acc[j], g[u][j], al);
        }
    });
}

template <int GH, int CH, bool VEC>
__global__ __launch_bounds__(256) void bwd_cols_kernel(Args a)
{
    const Lane ln(a);
    const int64_t row = group_index(a);
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row];
    int64_t d = (int64_t)a.rowptr[row + 1] - b;
    d = d < 0 ? 0 : d;
    if (d > kSeg) {
        if (blockIdx.y == 0 && ln.li == 0 && a.w.hubs.cap_hub > 0) append(a.w.hubs, (int32_t)row, d);
        return;
    }
    float4 xo[CH], acc[CH];
    load_own<CH, VEC>(ln, a.X + row * a.ldx, xo);
#pragma unroll
    for (int j = 0; j < CH; j++) acc[j] = zero4();
    float sum = 0.f;
    cols_entries<GH, CH, VEC>(a, ln, b, d, xo, a.colterm[row * a.cs + ln.hs], sum, acc);
#pragma unroll
    for (int j = 0; j < CH; j++) {
        if (!ln.has(j)) continue;
        float *dst = a.Y + row * a.ldy + ln.off(j);
        if (a.beta) acc[j] = add4(load_chunk<VEC>(dst, 0, ln.rem(j)), acc[j]);
        store_chunk<VEC>(dst, acc[j], ln.rem(j));
    }
    if (ln.first()) a.dterm[row * a.ds + ln.h] = sum;
}

template <int GH, int CH, bool VEC>
__global__ __launch_bounds__(256) void bwd_cols_seg_kernel(Args a)
{
    const Lane ln(a);
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        float4 xo[CH], acc[CH];
        load_own<CH, VEC>(ln, a.X + (int64_t)row * a.ldx, xo);
#pragma unroll
        for (int j = 0; j < CH; j++) acc[j] = zero4();
        float sum = 0.f;
        cols_entries<GH, CH, VEC>(a, ln, b, n, xo, a.colterm[(int64_t)row * a.cs + ln.hs], sum, acc);
#pragma unroll
        for (int j = 0; j < CH; j++)
            if (ln.has(j)) store_chunk<VEC>(a.w.part_f + slot * ((int64_t)a.H * a.D) + ln.off(j), acc[j], ln.rem(j));
        if (ln.first()) a.w.part_h[slot * a.H + ln.h] = sum;
    });
}

// the two counter words, cleared by a kernel (not a memset node: the call may be recorded into a graph)
__global__ void zero_counters_kernel(int32_t *counters)
{
    if (threadIdx.x < kCounters) counters[threadIdx.x] = 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Shape {
    int GH, GE, HP, CH;
    int64_t passes;
};

Shape shape_of(int32_t H, int32_t D)
{
    Shape s{};
    const int64_t Q = ((int64_t)D + 3) / 4;
    s.GH = 1;
    while (s.GH < Q && s.GH < 64) s.GH <<= 1;
    s.CH = (int)ceil_div(Q, s.GH);
    s.GE = s.GH;
    while (s.GE < 64 && s.GE < (int64_t)s.GH * H) s.GE <<= 1;
    s.HP = s.GE / s.GH;
    s.passes = ceil_div(H, s.HP);
    return s;
}

// what all three calls check before any HIP call
int check_common(int32_t n_rows, int32_t n_cols, int64_t nnz, int32_t H, int32_t D, const int32_t *rowptr, const int32_t *colidx, const float *rowterm,
                 int64_t rs, const float *colterm, int64_t cs, Shape *s)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(H >= 1 && D >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(rs >= H && cs >= H, GNNX_ERR_INVALID_ARG, "term stride < %d", H);
    GNNX_REQUIRE(nnz == 0 || (n_rows > 0 && n_cols > 0), GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    GNNX_REQUIRE(rowptr && rowterm && colterm && (nnz == 0 || colidx), GNNX_ERR_INVALID_ARG, "null pointer");
    *s = shape_of(H, D);
    GNNX_REQUIRE(s->CH <= kMaxChunks, GNNX_ERR_UNSUPPORTED, "head_dim %d > %d", D, 256 * kMaxChunks);
    GNNX_REQUIRE(s->passes < 65536 && (int64_t)H * D + H < (1ll << 31), GNNX_ERR_UNSUPPORTED, "%d heads of %d features are too many for one launch", H, D);
    return GNNX_OK;
}

dim3 rows_grid(int32_t n_rows, const Shape &s) { return dim3((uint32_t)ceil_div(n_rows, 256 / s.GE), (uint32_t)s.passes); }
dim3 seg_grid(const Work &w, const Shape &s)
{
    const int64_t groups = w.hubs.cap_seg < kSegGroups ? w.hubs.cap_seg : kSegGroups;
    return dim3((uint32_t)ceil_div(groups * s.GE, 256), (uint32_t)s.passes);
}
dim3 flat_grid(int64_t threads) { return dim3((uint32_t)ceil_div(threads < (1 << 24) ? threads : (1 << 24), 256)); }

// f(Int<CH>, bool_constant<VEC>) / f(Int<GH>, Int<CH>, bool_constant<VEC>) for the runtime shape
template <class F>
void with_chunks(const Shape &s, bool vec, F f)
{
    if (s.CH == 1) vec ? f(Int<1>{}, std::true_type{}) : f(Int<1>{}, std::false_type{});
    else vec ? f(Int<2>{}, std::true_type{}) : f(Int<2>{}, std::false_type{});
}
template <class F>
void with_shape(const Shape &s, bool vec, F f)
{
    auto go = [&](auto gh) {
        if (vec) f(gh, Int<1>{}, std::true_type{});
        else f(gh, Int<1>{}, std::false_type{});
    };
    switch (s.GH) {
    case 1: return go(Int<1>{});
    case 2: return go(Int<2>{});
    case 4: return go(Int<4>{});
    case 8: return go(Int<8>{});
    case 16: return go(Int<16>{});
    case 32: return go(Int<32>{});
    default:
        if (s.CH == 1) return go(Int<64>{});
        if (vec) f(Int<64>{}, Int<2>{}, std::true_type{});
        else f(Int<64>{}, Int<2>{}, std::false_type{});
    }
}

#define GAT_LAUNCH(kernel, grid) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a)

// The workspace every call requires is the neighbourhood reductions' (gnnx_spmm_csr_reduce_workspace) at width n_heads * (head_dim + 1):
// this unit adds no query of its own.  The carving above always fits it; `F` is what a segment slot writes per feature (0: row side).
int take_workspace(int32_t n_rows, int64_t nnz, int32_t H, int32_t D, int64_t F, void *d_workspace, size_t workspace_bytes, Work *w)
{
    size_t need = 0;
    int rc = gnnx_spmm_csr_reduce_workspace(n_rows, nnz, (int32_t)((int64_t)H * D + H), &need);
    if (rc) return rc;
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    GNNX_REQUIRE(256 + carve(n_rows, nnz, H, F, d_workspace, w) <= need, GNNX_ERR_WORKSPACE, "the attention lists do not fit the reduce workspace");
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_gat_aggregate_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, int32_t n_heads,
                                        int32_t head_dim, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm,
                                        int64_t colterm_stride, float negative_slope, const float *d_X, int64_t ldx, const float *d_bias, int relu_out,
                                        float *d_Y, int64_t ldy, float *d_rowmax, float *d_rowsum, void *d_workspace, size_t workspace_bytes,
                                        void *stream)
{
    Shape s;
    int rc = check_common(n_rows, n_cols, nnz, n_heads, head_dim, d_rowptr, d_colidx, d_rowterm, rowterm_stride, d_colterm, colterm_stride, &s);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldx >= F && ldy >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(d_Y && (nnz == 0 || d_X), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Args a{};
    rc = take_workspace(n_rows, nnz, n_heads, head_dim, F, d_workspace, workspace_bytes, &a.w);
    if (rc) return rc;
    a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.rowptr = d_rowptr, a.colidx = d_colidx;
    a.rowterm = d_rowterm, a.rs = rowterm_stride, a.colterm = d_colterm, a.cs = colterm_stride, a.slope = negative_slope;
    a.X = d_X, a.ldx = ldx, a.bias = d_bias, a.relu_out = relu_out != 0, a.Y = d_Y, a.ldy = ldy;
    a.rowmax_out = d_rowmax, a.rowsum_out = d_rowsum;
    a.GH = s.GH, a.GE = s.GE, a.HP = s.HP;
    const bool vec = head_dim % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(d_X) && aligned16(d_Y) && aligned16(d_bias);
    const bool hubs = a.w.hubs.cap_hub > 0;
    hipStream_t st = as_stream(stream);
    if (hubs) hipLaunchKernelGGL(zero_counters_kernel, dim3(1), dim3(64), 0, st, a.w.counters);
    with_chunks(s, vec, [&](auto ch, auto v) { GAT_LAUNCH((fwd_rows_kernel<decltype(ch)::value, decltype(v)::value>), rows_grid(n_rows, s)); });
    GNNX_LAUNCH_CHECK();
    if (hubs) {
        GAT_LAUNCH(fwd_seg_max_kernel, seg_grid(a.w, s));
        GAT_LAUNCH(hub_max_kernel, flat_grid(a.w.hubs.cap_hub * n_heads));
        with_chunks(s, vec, [&](auto ch, auto v) { GAT_LAUNCH((fwd_seg_acc_kernel<decltype(ch)::value, decltype(v)::value>), seg_grid(a.w, s)); });
        GAT_LAUNCH(hub_combine_kernel<0>, flat_grid(a.w.hubs.cap_hub * F));
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

GNNX_API int gnnx_gat_aggregate_bwd_rows_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                                 int32_t n_heads, int32_t head_dim, const float *d_rowterm, int64_t rowterm_stride,
                                                 const float *d_colterm, int64_t colterm_stride, float negative_slope, const float *d_G, int64_t ldg,
                                                 const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_bias,
                                                 const float *d_rowmax, const float *d_rowsum, float *d_drowterm, int64_t drowterm_stride,
                                                 float *d_dot, void *d_workspace, size_t workspace_bytes, void *stream)
{
    Shape s;
    int rc = check_common(n_rows, n_cols, nnz, n_heads, head_dim, d_rowptr, d_colidx, d_rowterm, rowterm_stride, d_colterm, colterm_stride, &s);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldx >= F && ldy >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(drowterm_stride >= n_heads, GNNX_ERR_INVALID_ARG, "drowterm stride < n_heads");
    GNNX_REQUIRE(d_G && d_Y && d_rowmax && d_rowsum && d_drowterm && d_dot && (nnz == 0 || d_X), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Args a{};
    rc = take_workspace(n_rows, nnz, n_heads, head_dim, 0, d_workspace, workspace_bytes, &a.w);
    if (rc) return rc;
    a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.rowptr = d_rowptr, a.colidx = d_colidx;
    a.rowterm = d_rowterm, a.rs = rowterm_stride, a.colterm = d_colterm, a.cs = colterm_stride, a.slope = negative_slope;
    a.X = d_X, a.ldx = ldx, a.G = d_G, a.ldg = ldg, a.Yin = d_Y, a.ldyin = ldy, a.bias = d_bias;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot_out = d_dot, a.dterm = d_drowterm, a.ds = drowterm_stride;
    a.GH = s.GH, a.GE = s.GE, a.HP = s.HP;
    const bool vec = head_dim % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(d_G) && aligned16(d_X) && aligned16(d_Y) &&
                     aligned16(d_bias);
    const bool hubs = a.w.hubs.cap_hub > 0;
    hipStream_t st = as_stream(stream);
    if (hubs) hipLaunchKernelGGL(zero_counters_kernel, dim3(1), dim3(64), 0, st, a.w.counters);
    with_shape(s, vec, [&](auto gh, auto ch, auto v) {
        GAT_LAUNCH((bwd_rows_kernel<decltype(gh)::value, decltype(ch)::value, decltype(v)::value>), rows_grid(n_rows, s));
        if (!hubs) return;
        GAT_LAUNCH((bwd_rows_seg_kernel<decltype(gh)::value, decltype(ch)::value, decltype(v)::value>), seg_grid(a.w, s));
        GAT_LAUNCH(hub_combine_kernel<2>, flat_grid(a.w.hubs.cap_hub * n_heads));
    });
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_gat_aggregate_bwd_cols_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                                 int32_t n_heads, int32_t head_dim, const float *d_rowterm, int64_t rowterm_stride,
                                                 const float *d_colterm, int64_t colterm_stride, float negative_slope, const float *d_G, int64_t ldg,
                                                 const float *d_X, int64_t ldx, const float *d_rowmax, const float *d_rowsum, const float *d_dot,
                                                 float beta, float *d_dX, int64_t lddx, float *d_dcolterm, int64_t dcolterm_stride,
                                                 void *d_workspace, size_t workspace_bytes, void *stream)
{
    Shape s;
    int rc = check_common(n_rows, n_cols, nnz, n_heads, head_dim, d_rowptr, d_colidx, d_rowterm, rowterm_stride, d_colterm, colterm_stride, &s);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldx >= F && lddx >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(dcolterm_stride >= n_heads, GNNX_ERR_INVALID_ARG, "dcolterm stride < n_heads");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE(d_X && d_dX && d_dcolterm && (nnz == 0 || (d_G && d_rowmax && d_rowsum && d_dot)), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Args a{};
    rc = take_workspace(n_rows, nnz, n_heads, head_dim, F, d_workspace, workspace_bytes, &a.w);
    if (rc) return rc;
    a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.rowptr = d_rowptr, a.colidx = d_colidx;
    a.rowterm = d_rowterm, a.rs = rowterm_stride, a.colterm = d_colterm, a.cs = colterm_stride, a.slope = negative_slope;
    a.X = d_X, a.ldx = ldx, a.G = d_G, a.ldg = ldg, a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot = d_dot;
    a.Y = d_dX, a.ldy = lddx, a.beta = beta != 0.f, a.dterm = d_dcolterm, a.ds = dcolterm_stride;
    a.GH = s.GH, a.GE = s.GE, a.HP = s.HP;
    const bool vec = head_dim % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && aligned16(d_G) && aligned16(d_X) && aligned16(d_dX);
    const bool hubs = a.w.hubs.cap_hub > 0;
    hipStream_t st = as_stream(stream);
    if (hubs) hipLaunchKernelGGL(zero_counters_kernel, dim3(1), dim3(64), 0, st, a.w.counters);
    with_shape(s, vec, [&](auto gh, auto ch, auto v) {
        GAT_LAUNCH((bwd_cols_kernel<decltype(gh)::value, decltype(ch)::value, decltype(v)::value>), rows_grid(n_rows, s));
        if (!hubs) return;
        GAT_LAUNCH((bwd_cols_seg_kernel<decltype(gh)::value, decltype(ch)::value, decltype(v)::value>), seg_grid(a.w, s));
        GAT_LAUNCH(hub_combine_kernel<1>, flat_grid(a.w.hubs.cap_hub * F));
    });
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}
