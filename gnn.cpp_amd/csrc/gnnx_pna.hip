// Principal Neighbourhood Aggregation (Corso et al. 2020): mean, min, max and standard deviation of the stored entries of each CSR row
// from ONE gather of the row, and the backward of all four from one walk of the transposed row -- include/gnnx.h "principal
// neighbourhood aggregation".
//   forward:   per row and feature  s1 = sum x, s2 = sum x * x, (max, argmax), (min, argmin)  ->  Y = mean | min | max | std
//   backward:  dX[c] (+)= sum over the entries q of row c of CSR(A^T) of  A_i + x_c B_i + routed dmax_i + routed dmin_i
// The sums have the header's order -- the forward an ascending chain from +0 per segment of S = 4096 entries, the backward a descending
// one, the segment sums added in ascending order -- and a maximum has none, so the bits are a function of the inputs alone.  How rows
// and segments map to lanes is gnnx_reduce.hip's:
//   * rows of d <= S entries: G = 4 .. 64 lanes per row, lane l owns features f0 .. f0 + VEC - 1 of tile blockIdx.y, the group fetches G
//     entries of the pattern with one coalesced load and hands them out by shuffle, four gathered rows are requested before the first
//     is consumed.  A forward lane carries s1, s2, (maxval, maxpos), (minval, minpos) per feature -- 24 registers of state with VEC = 4
//     beside the 16 of the gathered rows; a backward lane carries the two sums a and b and requests the six rows of four entries
//     (A, B, argmax, dmax, argmin, dmin) before the first add;
//   * hub rows, d > S: listed by the row kernel (gnnx_worklist.h), a fixed grid of lane groups strides over the segment slots and writes
//     each segment's six (two) words per feature to the workspace, a thread per (hub, feature) finishes the row in ascending order.
// MIN is MAX on the sign-flipped values, and the running value starts from the first entry: gnnx_reduce.hip's meet(), so min, max and
// both args are that unit's bits.  Division and square root are the compiler's correctly rounded ones (hipcc's default,
// -fhip-fp32-correctly-rounded-divide-sqrt; the Makefile passes no fast-math flag), no product is contracted into a sum.
// Every launch is on the caller's stream; nothing is allocated or synchronised.
#include "gnnx_lanes.h"
#include "gnnx_worklist.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kCounters = 16;     // int32 words in front of the workspace: [0], [1] the hub list's
constexpr int kSegGroups = 8192;  // lane groups of the segment kernels (stride over the slots)
constexpr uint32_t kSign = 0x80000000u;

// the caller's workspace, carved: NF float and NI int32 words per (segment slot, feature)
struct Lists {
    int32_t *counters;
    float *part_f[4];     // forward: s1, s2, maxval, minval (flipped); backward: a, b
    int32_t *part_i[2];   // forward: maxpos, minpos
    HubList hubs;
};

// bytes the carving takes from the first 256-byte boundary on: 4 * (16 + 2 hubs + segs + (NF + NI) segs F)
size_t carve(int32_t n_rows, int64_t nnz, int32_t F, int NF, int NI, void *ws, Lists *out)
{
    Lists w{};
    w.hubs.size(n_rows, nnz);
    Carver c(ws ? aligned_base(ws) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);   // 64 bytes: the partials stay 16-byte aligned (F % 4 == 0)
    for (int k = 0; k < NF; k++) w.part_f[k] = c.take<float>((size_t)w.hubs.cap_seg * F, 4);
    for (int k = 0; k < NI; k++) w.part_i[k] = c.take<int32_t>((size_t)w.hubs.cap_seg * F, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hubs.take_slots(c);
    if (out) *out = w;
    return c.bytes();
}

__device__ __forceinline__ float flip(float t) { return __uint_as_float(__float_as_uint(t) ^ kSign); }
__device__ __forceinline__ float4 flip(float4 t) { return make_float4(flip(t.x), flip(t.y), flip(t.z), flip(t.w)); }
__device__ __forceinline__ float sq(float x) { return x * x; }
__device__ __forceinline__ float4 sq(float4 x) { return make_float4(x.x * x.x, x.y * x.y, x.z * x.z, x.w * x.w); }

// ---- forward -------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    int32_t n_rows, F;
    const int32_t *rowptr, *colidx;
    const float *X;
    int64_t ldx;
    float eps;
    float *Y;             // mean at +0, min at +F, max at +2F, std at +3F of a row
    int64_t ldy;
    int32_t *argmin;
    int64_t ld_min;
    int32_t *argmax;
    int64_t ld_max;
};

// what a lane carries per feature
template <int VEC> struct Stats {
    typename Piece<VEC>::F s1, s2, maxv, minv;   // minv in the flipped domain
    typename Piece<VEC>::I maxp, minp;
};

template <int VEC> __device__ __forceinline__ void reset(Stats<VEC> &s)
{
    clear(s.s1);
    clear(s.s2);
    clear(s.maxv);
    clear(s.minv);
    none(s.maxp);
    none(s.minp);
}

// the header's chain from the row's sums: r = 1 / d, mean = s1 r, msq = s2 r, var = max(msq - mean mean, +0), std = sqrt(var + eps);
// a row without entries gives +0 twice
__device__ __forceinline__ void moments(float s1, float s2, int64_t d, float eps, float &mean, float &sd)
{
    if (d == 0) {
        mean = 0.f;
        sd = 0.f;
        return;
    }
    const float r = 1.0f / (float)d;
    mean = s1 * r;
    const float msq = s2 * r;
    const float mm = mean * mean;
    const float diff = msq - mm;
    const float var = diff > 0.f ? diff : 0.f;
    sd = sqrtf(var + eps);
}
__device__ __forceinline__ void moments(float4 s1, float4 s2, int64_t d, float eps, float4 &mean, float4 &sd)
{
    moments(s1.x, s2.x, d, eps, mean.x, sd.x);
    moments(s1.y, s2.y, d, eps, mean.y, sd.y);
    moments(s1.z, s2.z, d, eps, mean.z, sd.z);
    moments(s1.w, s2.w, d, eps, mean.w, sd.w);
}

// the winner with its own bits, +0 where the row has no entry (flipped: the value lives in the sign-flipped domain)
__device__ __forceinline__ float stored(float val, int32_t pos, bool flipped) { return pos < 0 ? 0.f : flipped ? flip(val) : val; }
__device__ __forceinline__ float4 stored(float4 v, int4 p, bool f)
{
    return make_float4(stored(v.x, p.x, f), stored(v.y, p.y, f), stored(v.z, p.z, f), stored(v.w, p.w, f));
}

// B entries k .. k + B - 1 of the group's current window (positions lo + k, ...): all loads, then the four updates in ascending position
template <int G, int VEC, int B>
__device__ __forceinline__ void fwd_batch(Stats<VEC> &s, int k, int64_t lo, int32_t myc, int gbase, const float *xf, const FwdArgs &a)
{
    using V = typename Piece<VEC>::F;
    int32_t c[B];
    V x[B];
#pragma unroll
    for (int u = 0; u < B; u++) c[u] = __shfl(myc, gbase + k + u, 64);
#pragma unroll
    for (int u = 0; u < B; u++) x[u] = *reinterpret_cast<const V *>(xf + (int64_t)c[u] * a.ldx);
#pragma unroll
    for (int u = 0; u < B; u++) {
        const int32_t p = (int32_t)(lo + k + u);
        s.s1 = add(s.s1, x[u]);
        s.s2 = add(s.s2, sq(x[u]));
        meet(s.maxv, s.maxp, x[u], p);
        meet(s.minv, s.minp, flip(x[u]), p);
    }
}

// the entries b .. e - 1 in ascending position; every lane of the group runs every shuffle
template <int G, int VEC>
__device__ __forceinline__ void fwd_span(Stats<VEC> &s, int64_t b, int64_t e, int li, int gbase, const float *xf, const FwdArgs &a)
{
    for (int64_t lo = b; lo < e; lo += G) {
        int64_t q = lo + li;
        q = q < e ? q : e - 1;
        const int32_t myc = a.colidx[q];
        const int n = e - lo < G ? (int)(e - lo) : G;
        int k = 0;
        for (; k + 4 <= n; k += 4) fwd_batch<G, VEC, 4>(s, k, lo, myc, gbase, xf, a);
        for (; k < n; k++) fwd_batch<G, VEC, 1>(s, k, lo, myc, gbase, xf, a);
    }
}

// what a lane group of the row and segment kernels knows of itself
struct Lane {
    int li, gbase;
    int64_t f0, fa;   // the lane's first feature; the one it reads (0 for a lane past the row, which never stores)
    bool active;
};
template <int G, int VEC> __device__ __forceinline__ Lane lane_of(int32_t F)
{
    Lane l;
    l.li = threadIdx.x % G;
    l.gbase = (threadIdx.x & 63) - l.li;
    l.f0 = ((int64_t)blockIdx.y * G + l.li) * VEC;
    l.active = l.f0 < F;               // VEC == 4: F % 4 == 0, so the whole piece is inside the row
    l.fa = l.active ? l.f0 : 0;
    return l;
}

// grid.x: blocks of 256 / G rows; grid.y: tiles of G * VEC features.  A row longer than S goes to the hub list (tile 0 lists it).
template <int G, int VEC>
__global__ __launch_bounds__(256) void fwd_rows_kernel(FwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    constexpr int GROUPS = 256 / G;
    const Lane l = lane_of<G, VEC>(a.F);
    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (row >= a.n_rows) return;                // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (l.li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    Stats<VEC> s;
    reset(s);
    fwd_span<G, VEC>(s, b, e, l.li, l.gbase, a.X + l.fa, a);
    if (!l.active) return;
    V mean, sd;
    moments(s.s1, s.s2, e - b, a.eps, mean, sd);
    float *y = a.Y + row * a.ldy + l.f0;
    *reinterpret_cast<V *>(y) = mean;
    *reinterpret_cast<V *>(y + a.F) = stored(s.minv, s.minp, true);
    *reinterpret_cast<V *>(y + 2 * (int64_t)a.F) = stored(s.maxv, s.maxp, false);
    *reinterpret_cast<V *>(y + 3 * (int64_t)a.F) = sd;
    if (a.argmin) *reinterpret_cast<P *>(a.argmin + row * a.ld_min + l.f0) = s.minp;
    if (a.argmax) *reinterpret_cast<P *>(a.argmax + row * a.ld_max + l.f0) = s.maxp;
}

// The lane groups of the segment kernels stride over the hub list's slots.  body(b, e, at): the segment's entries b .. e - 1 and the
// place of (slot, the lane's first feature) in the partials.
template <int G, class Body>
__device__ __forceinline__ void for_group_segments(const int32_t *__restrict__ rowptr, int32_t F, const Lists &w, const Lane &l, Body body)
{
    constexpr int GROUPS = 256 / G;
    for_hub_segments(w.hubs, rowptr, (int64_t)blockIdx.x * GROUPS + threadIdx.x / G, (int64_t)gridDim.x * GROUPS,
                     [&](int32_t, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) { body(b, b + n, slot * F + l.f0); });
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void fwd_seg_kernel(FwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    const Lane l = lane_of<G, VEC>(a.F);
    for_group_segments<G>(a.rowptr, a.F, w, l, [&](int64_t b, int64_t e, int64_t at) {
        Stats<VEC> s;
        reset(s);
        fwd_span<G, VEC>(s, b, e, l.li, l.gbase, a.X + l.fa, a);
        if (l.active) {
            *reinterpret_cast<V *>(w.part_f[0] + at) = s.s1;
            *reinterpret_cast<V *>(w.part_f[1] + at) = s.s2;
            *reinterpret_cast<V *>(w.part_f[2] + at) = s.maxv;
            *reinterpret_cast<V *>(w.part_f[3] + at) = s.minv;
            *reinterpret_cast<P *>(w.part_i[0] + at) = s.maxp;
            *reinterpret_cast<P *>(w.part_i[1] + at) = s.minp;
        }
    });
}

// a thread per (hub, feature): the segment sums are added and the segment winners meet in ascending order (of equal values the
// smaller position stays), then the row's chain
__global__ __launch_bounds__(256) void fwd_combine_kernel(FwdArgs a, Lists w)
{
    const int64_t total = listed_hubs(w.hubs) * a.F;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t h = idx / a.F, f = idx - h * a.F;
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t d = (int64_t)a.rowptr[row + 1] - a.rowptr[row];
        const int64_t nseg = (d + kSeg - 1) / kSeg;
        const int64_t at = (int64_t)w.hubs.hub_seg0[h] * a.F + f;
        float s1 = w.part_f[0][at], s2 = w.part_f[1][at], maxv = 0.f, minv = 0.f;
        int32_t maxp = -1, minp = -1;
        for (int64_t s = 0; s < nseg; s++) {
            const int64_t x = at + s * a.F;
            if (s > 0) {
                s1 = s1 + w.part_f[0][x];
                s2 = s2 + w.part_f[1][x];
            }
            meet(maxv, maxp, w.part_f[2][x], w.part_i[0][x]);
            meet(minv, minp, w.part_f[3][x], w.part_i[1][x]);
        }
        float mean, sd;
        moments(s1, s2, d, a.eps, mean, sd);
        float *y = a.Y + (int64_t)row * a.ldy + f;
        y[0] = mean;
        y[a.F] = stored(minv, minp, true);
        y[2 * (int64_t)a.F] = stored(maxv, maxp, false);
        y[3 * (int64_t)a.F] = sd;
        if (a.argmin) a.argmin[(int64_t)row * a.ld_min + f] = minp;
        if (a.argmax) a.argmax[(int64_t)row * a.ld_max + f] = maxp;
    }
}

// ---- backward: the per-row coefficients ----------------------------------------------------------------------------------------
struct CoeffArgs {
    int32_t n_rows, F;
    const int32_t *rowptr;
    const float *Y;       // the forward's output: mean at +0, std at +3F
    int64_t ldy;
    const float *dM;      // its gradient: dmean at +0, dstd at +3F
    int64_t ldm;
    float *A, *B;
    int64_t lda, ldb;
};

// B = (dstd r) / std;  A = dmean r - B mean: one rounding per written operation
__device__ __forceinline__ void coeff(float mean, float sd, float dmean, float dstd, float r, float &A, float &B)
{
    const float t = dstd * r;
    B = t / sd;
    const float u = dmean * r;
    const float v = B * mean;
    A = u - v;
}

// a lane per (row, piece of VEC features), rows streamed in order: four coalesced reads and two writes per piece
template <int VEC>
__global__ __launch_bounds__(256) void coeff_kernel(CoeffArgs a)
{
    using V = typename Piece<VEC>::F;
    const int64_t pieces = a.F / VEC, total = (int64_t)a.n_rows * pieces;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t row = idx / pieces, f = (idx - row * pieces) * VEC;
        const int32_t d = a.rowptr[row + 1] - a.rowptr[row];
        V A, B;
        clear(A);
        clear(B);
        if (d > 0) {
            const float r = 1.0f / (float)d;
            const float *y = a.Y + row * a.ldy + f, *g = a.dM + row * a.ldm + f;
            const V mean = *reinterpret_cast<const V *>(y), sd = *reinterpret_cast<const V *>(y + 3 * (int64_t)a.F);
            const V dmean = *reinterpret_cast<const V *>(g), dstd = *reinterpret_cast<const V *>(g + 3 * (int64_t)a.F);
            if constexpr (VEC == 4) {
                coeff(mean.x, sd.x, dmean.x, dstd.x, r, A.x, B.x);
                coeff(mean.y, sd.y, dmean.y, dstd.y, r, A.y, B.y);
                coeff(mean.z, sd.z, dmean.z, dstd.z, r, A.z, B.z);
                coeff(mean.w, sd.w, dmean.w, dstd.w, r, A.w, B.w);
            } else {
                coeff(mean, sd, dmean, dstd, r, A, B);
            }
        }
        *reinterpret_cast<V *>(a.A + row * a.lda + f) = A;
        *reinterpret_cast<V *>(a.B + row * a.ldb + f) = B;
    }
}

// ---- backward: the walk of the transposed rows ---------------------------------------------------------------------------------
struct BwdArgs {
    int32_t n_rows, F;            // of the transposed pattern
    const int32_t *rowptr, *colidx, *map;
    const float *A, *B;
    int64_t lda, ldb;
    const int32_t *argmin, *argmax;
    int64_t ld_min, ld_max;
    const float *dM;              // dmin at +F, dmax at +2F of a row, read in place
    int64_t ldm;
    const float *X;
    int64_t ldx;
    int beta;
    float *dX;
    int64_t lddx;
};

// acc + t where the entry won the feature, acc itself where it did not
__device__ __forceinline__ float route(float acc, float t, int32_t won, int32_t p) { return won == p ? acc + t : acc; }
__device__ __forceinline__ float4 route(float4 acc, float4 t, int4 won, int32_t p)
{
    return make_float4(route(acc.x, t.x, won.x, p), route(acc.y, t.y, won.y, p), route(acc.z, t.z, won.z, p), route(acc.w, t.w, won.w, p));
}
__device__ __forceinline__ float axb(float a, float x, float b) { const float t = x * b; return a + t; }
__device__ __forceinline__ float4 axb(float4 a, float4 x, float4 b) { return make_float4(axb(a.x, x.x, b.x), axb(a.y, x.y, b.y), axb(a.z, x.z, b.z), axb(a.w, x.w, b.w)); }

// B entries k .. k + B - 1 from the top of the group's current window: all six rows of every entry, then per entry A, max, min and B
template <int G, int VEC, int B>
__device__ __forceinline__ void bwd_batch(typename Piece<VEC>::F &sa, typename Piece<VEC>::F &sb, int k, int32_t myi, int32_t myp, int gbase,
                                          int64_t fa, const BwdArgs &a)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    int32_t i[B], p[B];
    V ca[B], cb[B], gmax[B], gmin[B];
    P wmax[B], wmin[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
        i[u] = __shfl(myi, gbase + k + u, 64);
        p[u] = __shfl(myp, gbase + k + u, 64);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
        const float *g = a.dM + (int64_t)i[u] * a.ldm + fa;
        ca[u] = *reinterpret_cast<const V *>(a.A + (int64_t)i[u] * a.lda + fa);
        cb[u] = *reinterpret_cast<const V *>(a.B + (int64_t)i[u] * a.ldb + fa);
        wmax[u] = *reinterpret_cast<const P *>(a.argmax + (int64_t)i[u] * a.ld_max + fa);
        gmax[u] = *reinterpret_cast<const V *>(g + 2 * (int64_t)a.F);
        wmin[u] = *reinterpret_cast<const P *>(a.argmin + (int64_t)i[u] * a.ld_min + fa);
        gmin[u] = *reinterpret_cast<const V *>(g + a.F);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
        sa = add(sa, ca[u]);
        sa = route(sa, gmax[u], wmax[u], p[u]);
        sa = route(sa, gmin[u], wmin[u], p[u]);
        sb = add(sb, cb[u]);
    }
}

// two accumulators per feature over the entries e - 1 down to b
template <int G, int VEC>
__device__ __forceinline__ void bwd_span(typename Piece<VEC>::F &sa, typename Piece<VEC>::F &sb, int64_t b, int64_t e, const Lane &l, const BwdArgs &a)
{
    for (int64_t hi = e; hi > b; hi -= G) {
        int64_t q = hi - 1 - l.li;
        q = q >= b ? q : b;
        const int32_t myi = a.colidx[q], myp = a.map[q];
        const int n = hi - b < G ? (int)(hi - b) : G;
        int k = 0;
        for (; k + 4 <= n; k += 4) bwd_batch<G, VEC, 4>(sa, sb, k, myi, myp, l.gbase, l.fa, a);
        for (; k < n; k++) bwd_batch<G, VEC, 1>(sa, sb, k, myi, myp, l.gbase, l.fa, a);
    }
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void bwd_rows_kernel(BwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    constexpr int GROUPS = 256 / G;
    const Lane l = lane_of<G, VEC>(a.F);
    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (l.li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    V sa, sb;
    clear(sa);
    clear(sb);
    bwd_span<G, VEC>(sa, sb, b, e, l, a);
    if (!l.active) return;
    const V t = axb(sa, *reinterpret_cast<const V *>(a.X + row * a.ldx + l.f0), sb);
    V *dst = reinterpret_cast<V *>(a.dX + row * a.lddx + l.f0);
    V base;
    clear(base);
    if (a.beta) base = *dst;
    *dst = add(base, t);
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void bwd_seg_kernel(BwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    const Lane l = lane_of<G, VEC>(a.F);
    for_group_segments<G>(a.rowptr, a.F, w, l, [&](int64_t b, int64_t e, int64_t at) {
        V sa, sb;
        clear(sa);
        clear(sb);
        bwd_span<G, VEC>(sa, sb, b, e, l, a);
        if (l.active) {
            *reinterpret_cast<V *>(w.part_f[0] + at) = sa;
            *reinterpret_cast<V *>(w.part_f[1] + at) = sb;
        }
    });
}

// a thread per (hub, feature): ((seg_0 + seg_1) + seg_2) + ... for a and for b, then the store
__global__ __launch_bounds__(256) void bwd_combine_kernel(BwdArgs a, Lists w)
{
    const int64_t total = listed_hubs(w.hubs) * a.F;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t h = idx / a.F, f = idx - h * a.F;
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t at = (int64_t)w.hubs.hub_seg0[h] * a.F + f;
        float sa = w.part_f[0][at], sb = w.part_f[1][at];
        for (int64_t s = 1; s < nseg; s++) {
            sa = sa + w.part_f[0][at + s * a.F];
            sb = sb + w.part_f[1][at + s * a.F];
        }
        const float t = axb(sa, a.X[(int64_t)row * a.ldx + f], sb);
        float *dst = a.dX + (int64_t)row * a.lddx + f;
        *dst = (a.beta ? *dst : 0.f) + t;
    }
}

// ---- launch chains -------------------------------------------------------------------------------------------------------------
struct Shape {
    bool vec;
    int G;
    uint32_t tiles;
};

inline Shape shape_of(int32_t F, bool vec)
{
    const int64_t lanes = vec ? F / 4 : F;
    const int G = lanes > 32 ? 64 : lanes > 16 ? 32 : lanes > 8 ? 16 : lanes > 4 ? 8 : 4;
    return Shape{vec, G, (uint32_t)ceil_div(lanes, G)};
}

inline uint32_t seg_blocks(const HubList &w, int G) { return (uint32_t)ceil_div(w.cap_seg < kSegGroups ? w.cap_seg : kSegGroups, 256 / G); }
inline uint32_t combine_blocks(const HubList &w, int32_t F) { return (uint32_t)ceil_div(w.cap_hub * F < (1 << 19) ? w.cap_hub * F : (1 << 19), 256); }

template <int G, int VEC>
int launch_fwd(const FwdArgs &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    hipLaunchKernelGGL((fwd_rows_kernel<G, VEC>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), tiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((fwd_seg_kernel<G, VEC>), dim3(seg_blocks(w.hubs, G), tiles), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(fwd_combine_kernel, dim3(combine_blocks(w.hubs, a.F)), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

template <int G, int VEC>
int launch_bwd(const BwdArgs &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    hipLaunchKernelGGL((bwd_rows_kernel<G, VEC>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), tiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((bwd_seg_kernel<G, VEC>), dim3(seg_blocks(w.hubs, G), tiles), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(bwd_combine_kernel, dim3(combine_blocks(w.hubs, a.F)), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

#define GNNX_DISPATCH_SHAPE(LAUNCH, sh, ...)                                                         \
    switch ((sh).G) {                                                                                \
    case 4: return (sh).vec ? LAUNCH<4, 4>(__VA_ARGS__) : LAUNCH<4, 1>(__VA_ARGS__);                 \
    case 8: return (sh).vec ? LAUNCH<8, 4>(__VA_ARGS__) : LAUNCH<8, 1>(__VA_ARGS__);                 \
    case 16: return (sh).vec ? LAUNCH<16, 4>(__VA_ARGS__) : LAUNCH<16, 1>(__VA_ARGS__);              \
    case 32: return (sh).vec ? LAUNCH<32, 4>(__VA_ARGS__) : LAUNCH<32, 1>(__VA_ARGS__);              \
    default: return (sh).vec ? LAUNCH<64, 4>(__VA_ARGS__) : LAUNCH<64, 1>(__VA_ARGS__);              \
    }

// what every entry point checks before any device call
int check_sizes(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_feat >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    return GNNX_OK;
}

inline bool lines16(int64_t ld, const void *p) { return ld % 4 == 0 && aligned16(p); }   // every row of the matrix may be read as float4s

}  // namespace

GNNX_API int gnnx_spmm_csr_pna_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                   const float *d_X, int64_t ldx, float eps, float *d_Y, int64_t ldy, int32_t *d_argmin, int64_t ld_argmin,
                                   int32_t *d_argmax, int64_t ld_argmax, void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows, n_cols, n_feat, nnz);
    if (rc) return rc;
    GNNX_REQUIRE(eps >= 0.f, GNNX_ERR_INVALID_ARG, "eps must be >= 0");
    GNNX_REQUIRE(ldx >= n_feat && (!d_argmin || ld_argmin >= n_feat) && (!d_argmax || ld_argmax >= n_feat), GNNX_ERR_INVALID_ARG, "ld < n_feat");
    GNNX_REQUIRE(ldy >= 4 * (int64_t)n_feat, GNNX_ERR_INVALID_ARG, "ldy < 4 * n_feat");
    if (n_rows == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr && d_Y && (nnz == 0 || (d_colidx && d_X)), GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    const size_t need = 256 + carve(n_rows, nnz, n_feat, 4, 2, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    const bool vec = n_feat % 4 == 0 && lines16(ldx, d_X) && lines16(ldy, d_Y) && (!d_argmin || lines16(ld_argmin, d_argmin)) &&
                     (!d_argmax || lines16(ld_argmax, d_argmax));
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    hipStream_t st = as_stream(stream);
    const FwdArgs a{n_rows, n_feat, d_rowptr, d_colidx, d_X, ldx, eps, d_Y, ldy, d_argmin, ld_argmin, d_argmax, ld_argmax};
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    GNNX_DISPATCH_SHAPE(launch_fwd, sh, a, w, sh.tiles, st)
}

GNNX_API int gnnx_pna_bwd_coeff_f32(int32_t n_rows, int32_t n_feat, const int32_t *d_rowptr, const float *d_Y, int64_t ldy, const float *d_dM,
                                    int64_t ldm, float *d_A, int64_t lda, float *d_B, int64_t ldb, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_feat >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(lda >= n_feat && ldb >= n_feat, GNNX_ERR_INVALID_ARG, "ld < n_feat");
    GNNX_REQUIRE(ldy >= 4 * (int64_t)n_feat && ldm >= 4 * (int64_t)n_feat, GNNX_ERR_INVALID_ARG, "ldy or ldm < 4 * n_feat");
    if (n_rows == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(d_rowptr && d_Y && d_dM && d_A && d_B, GNNX_ERR_INVALID_ARG, "null pointer");
    const bool vec = n_feat % 4 == 0 && lines16(ldy, d_Y) && lines16(ldm, d_dM) && lines16(lda, d_A) && lines16(ldb, d_B);
    const CoeffArgs a{n_rows, n_feat, d_rowptr, d_Y, ldy, d_dM, ldm, d_A, d_B, lda, ldb};
    const int64_t lanes = (int64_t)n_rows * (vec ? n_feat / 4 : n_feat);
    const dim3 grid((uint32_t)ceil_div(lanes < (1 << 22) ? lanes : (1 << 22), 256));
    if (vec)
        hipLaunchKernelGGL(coeff_kernel<4>, grid, dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(coeff_kernel<1>, grid, dim3(256), 0, as_stream(stream), a);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_spmm_csr_pna_bwd_f32(int32_t n_rows_t, int32_t n_cols_t, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr_t,
                                       const int32_t *d_colidx_t, const int32_t *d_map_t, const float *d_A, int64_t lda, const float *d_B,
                                       int64_t ldb, const int32_t *d_argmin, int64_t ld_argmin, const int32_t *d_argmax, int64_t ld_argmax,
                                       const float *d_dM, int64_t ldm, const float *d_X, int64_t ldx, float beta, float *d_dX, int64_t lddx,
                                       void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows_t, n_cols_t, n_feat, nnz);
    if (rc) return rc;
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE(lda >= n_feat && ldb >= n_feat && ld_argmin >= n_feat && ld_argmax >= n_feat && ldx >= n_feat && lddx >= n_feat,
                 GNNX_ERR_INVALID_ARG, "ld < n_feat");
    GNNX_REQUIRE(ldm >= 4 * (int64_t)n_feat, GNNX_ERR_INVALID_ARG, "ldm < 4 * n_feat");
    if (n_rows_t == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols_t > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr_t && d_X && d_dX && (nnz == 0 || (d_colidx_t && d_map_t && d_A && d_B && d_argmin && d_argmax && d_dM)),
                 GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    const size_t need = 256 + carve(n_rows_t, nnz, n_feat, 2, 0, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    const bool vec = n_feat % 4 == 0 && lines16(lda, d_A) && lines16(ldb, d_B) && lines16(ld_argmin, d_argmin) && lines16(ld_argmax, d_argmax) &&
                     lines16(ldm, d_dM) && lines16(ldx, d_X) && lines16(lddx, d_dX);
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    hipStream_t st = as_stream(stream);
    const BwdArgs a{n_rows_t, n_feat, d_rowptr_t, d_colidx_t, d_map_t, d_A, d_B, lda, ldb, d_argmin, d_argmax, ld_argmin, ld_argmax,
                    d_dM, ldm, d_X, ldx, beta != 0.f, d_dX, lddx};
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    GNNX_DISPATCH_SHAPE(launch_bwd, sh, a, w, sh.tiles, st)
}
