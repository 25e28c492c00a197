// Dot-product (transformer) attention over CSR rows with optional edge features -- include/gnnx.h "dot-product attention".  Per head
// of width D, for entry p of row i with c = colidx[p] and e = eidx[p]:
//   k'_p = K[c] + E[e];  v'_p = V[c] + E[e];  s_p = scale * <Q[i], k'_p>;  m_i = max_p s_p;  x_p = expf(s_p - m_i);  z_i = sum_p x_p
//   forward    Y[i] = (sum_p x_p v'_p) / z_i,  rowmax = m,  rowsum = z
//   bwd, rows  dot[i, h] = <G_i, Y_i>_h;  dQ[i] = scale * sum_p ds_p k'_p;  dE[e_p] = alpha_p G_i + (scale * ds_p) Q_i   (forward pattern)
//   bwd, cols  dV[c] (+)= sum_i alpha_ic G_i;  dK[c] (+)= scale * sum_i ds_ic Q_i                                    (transposed pattern)
// with alpha_p = x_p / z_i, dalpha_p = <G_i, v'_p>, ds_p = alpha_p (dalpha_p - dot).  No transpose map, no [nnz, .] array, no atomic on a
// value.  The fused GAT calls (gnnx_gat_fused.hip) find the row maximum in a scalar sweep before they gather a feature row; here the score
// IS a D-wide dot product with the gathered row, so a max-first sweep would gather K (and E) twice.  The forward therefore runs an ONLINE
// softmax and gathers every row once.
//
// ORDER (the contract; a function of the row length and of D alone).  A row is cut into segments of S = 4096 consecutive entries (a row
// of d <= S entries is one segment); a segment is walked in ascending order in BLOCKS of 4 consecutive entries, the last block holding
// the 1 .. 4 entries that are left.  Every dot product over a head's D features is the order of gnnx_edge_dot.h with F := D (left
// operand Q for s, G for dot and dalpha), then s takes one multiply by scale.
//   forward, a segment from (m, z, N) = (-inf, +0, +0):  per block  m' = max(m, s_u);  r = (m == m') ? 1 : expf(m - m');
//     z = z * r, then z = z + x_u for u ascending with x_u = expf(s_u - m');  N[f] = N[f] * r, then N[f] = N[f] + (x_u * v'_u[f]);  m = m'.
//     One segment: Y = N / z (one IEEE division; an empty row: Y = +0, m = -inf, z = +0).  Several: m = max_s m_s,
//     w_s = (m_s == m) ? 1 : expf(m_s - m), z = (z_0 * w_0) + (z_1 * w_1) + ... ascending, N[f] likewise, Y = N / z.
//   backward: m and z are operands, so nothing is rescaled: ONE accumulator per output element from +0 over a segment's entries ascending
//     (each product rounded first), the segments' sums added ascending from the first, then dQ and dK take one multiply by scale.
//     alpha = expf(s - m) / z is one expf and one division; dE[e, f] = (alpha * G[f]) + ((scale * ds) * Q[f]).
// How rows, heads and features map to lanes is not in the result.
//
// LANES.  A head is a group of GH = min(64, pow2 >= ceil(D / 4)) lanes, each owning ONE 16-byte chunk of the head's slab (so D <= 256);
// a row is a group of GE = max(4, min(64, pow2 >= GH H)) lanes holding GE / GH heads, further heads are passes in grid.y; a head never
// straddles a group (GE >= 4 so that a window of GE indices is whole blocks -- the block structure must not depend on H).  The kernels are
// instantiated on GH: the head's lane, its chunk and the butterfly's stages are compile-time, which gnnx_gat_fused.hip names as its open
// cost.  The own row's Q (and G) chunk stays in registers for the whole row.  The group loads GE column indices and GE edge indices with
// one coalesced load each and hands them out by shuffle; a block requests its four K, E and V chunks (12 loads a lane) before the first
// is consumed, computes the four partial dots and runs the four xor butterflies interleaved.  One expf per entry plus one per block.
// Chunks that cannot be loaded as 16 bytes (D % 4 != 0, a pointer or pitch off 16 bytes) go through load_chunk<false> into the SAME chunk
// layout: one source, one order, same bits.
// HUBS (d > S).  The row kernel lists them (gnnx_worklist.h) and leaves them alone; lane groups of a fixed grid stride over the segment
// slots and write (m_s, z_s, N_s[F]) per slot in ONE pass (the fused GAT forward needs two); a thread per (hub, element) combines.  The
// backward calls need one segment pass and a plain ascending add.  All of it is skipped on the host when nnz <= S.
// No matrix instruction fits: there is no operand reuse, the work is a gather with about 4 flops per gathered float.
// Every loop is bounded by a row or segment length read from rowptr; nothing waits on another workgroup.
#include "gnnx_edge_dot.h"
#include "gnnx_worklist.h"

#include <type_traits>

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kCounters = 16;      // int32 words in front of the workspace: [0], [1] the hub list's
constexpr int kSegGroups = 8192;   // lane groups of a segment pass (stride over the slots)
constexpr int kBlock = 4;          // entries of a block of the walk (the contract's)
constexpr int kMaxDim = 256;       // one 16-byte chunk per lane, 64 lanes per head

struct Work {
    int32_t *counters;
    HubList hubs;
    float *part_f;   // [cap_seg, 2 F] per slot: N_s (forward), the dQ partial (row side), the dV | dK partials (column side)
    float *part_h;   // [cap_seg, 2 H] per slot: m_s | z_s (forward)
};

// The caller's pointer is aligned to 256 bytes and the counters take 64, so part_f is stored in 16-byte chunks.
size_t carve(int32_t n_rows, int64_t nnz, int32_t H, int64_t F, void *base, Work *out)
{
    Work w{};
    w.hubs.size(n_rows, nnz);
    Carver c(base ? aligned_base(base) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);
    w.part_f = c.take<float>((size_t)w.hubs.cap_seg * 2 * F, 16);
    w.part_h = c.take<float>((size_t)w.hubs.cap_seg * 2 * H, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hubs.take_slots(c);
    if (out) *out = w;
    return c.bytes();
}

// One struct for the three calls.  "own" is the row of the pattern the call runs on, "gathered" the entry's column.
struct Args {
    int32_t n_rows, H, D;
    const int32_t *rowptr, *colidx, *eidx;
    float scale;
    const float *Q, *K, *V, *E, *G, *Yin;     // forward and row side: Q, G, Yin own, K, V gathered; column side: K, V own, Q, G gathered
    int64_t ldq, ldk, ldv, lde, ldg, ldyin;
    const float *rowmax, *rowsum, *dot;        // backward inputs, [n, H] (dot: column side)
    float *rowmax_out, *rowsum_out, *dot_out;  // forward outputs; row side: dot
    float *A, *B, *dE;                         // forward: Y; row side: dQ; column side: dV, dK
    int64_t lda, ldb, ldde;
    int beta;
    int32_t GE, HP;                            // lanes per row, heads per pass
    Work w;
};

template <int N> using Int = std::integral_constant<int, N>;

__device__ __forceinline__ float4 mul_add(float4 acc, float4 x, float v)   // each product rounded, then the sum
{
    return make_float4(acc.x + (x.x * v), acc.y + (x.y * v), acc.z + (x.z * v), acc.w + (x.w * v));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float v) { return make_float4(a.x * v, a.y * v, a.z * v, a.w * v); }
__device__ __forceinline__ float4 div4(float4 a, float v)
{
    return make_float4(__fdiv_rn(a.x, v), __fdiv_rn(a.y, v), __fdiv_rn(a.z, v), __fdiv_rn(a.w, v));
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float rescale_of(float m, float m_new) { return m == m_new ? 1.f : expf(m - m_new); }

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

// where a lane stands: in its row's group, in its head's group, and the chunk it owns
template <int GH>
struct Lane {
    int li, gbase;
    int32_t h, hs, rem;   // the head; the head whose scalars the lane reads; features of the head from the chunk on
    int64_t off;          // the chunk's first feature in a row
    bool has, first;      // the lane owns a chunk; the lane stores the head's scalars
    __device__ __forceinline__ explicit Lane(const Args &a)
    {
        li = threadIdx.x & (a.GE - 1);
        gbase = (threadIdx.x & 63) - li;
        const int lh = li & (GH - 1);
        h = (int32_t)blockIdx.y * a.HP + li / GH;
        const bool head_ok = h < a.H;
        hs = head_ok ? h : 0;   // lanes without a head read head 0's scalars and store nothing
        rem = a.D - 4 * lh;
        has = head_ok && rem > 0;
        first = head_ok && lh == 0;
        off = (int64_t)hs * a.D + 4 * lh;
    }
    template <bool VEC>
    __device__ __forceinline__ float4 load(const float *row) const { return has ? load_chunk<VEC>(row + off, 0, rem) : zero4(); }
    template <bool VEC>
    __device__ __forceinline__ void store(float *row, const float4 &v) const { if (has) store_chunk<VEC>(row + off, v, rem); }
    template <bool VEC>   // the lane's share of a head's dot product: its chunk's products ascending into one accumulator from +0
    __device__ __forceinline__ float partial(const float4 &l, const float4 &r) const { return has ? add_chunk<VEC>(0.f, l, r, 0, rem) : 0.f; }
};

// N butterflies over the head's GH lanes, interleaved stage by stage: every lane of the head ends with the same bits
template <int GH, int N>
__device__ __forceinline__ void butterflies(float (&v)[N])
{
#pragma unroll
    for (int s = 1; s < GH; s <<= 1) {
        float o[N];
#pragma unroll
        for (int u = 0; u < N; u++) o[u] = __shfl_xor(v[u], s, 64);
#pragma unroll
        for (int u = 0; u < N; u++) v[u] = v[u] + o[u];
    }
}

// the lane group that runs the row (row kernels) or strides over the segment slots (segment kernels)
__device__ __forceinline__ int64_t group_index(const Args &a) { return ((int64_t)blockIdx.x * 256 + threadIdx.x) / a.GE; }
__device__ __forceinline__ int64_t group_count(const Args &a) { return (int64_t)gridDim.x * 256 / a.GE; }

// body(cnt, c[4], e[4]) for the blocks of the entries b .. b + n - 1 in ascending order: cnt = 4 entries, 1 .. 4 in the last block,
// whose c[u], e[u] for u >= cnt repeat its last entry (loadable, never consumed).  GE is a multiple of 4, so a window of GE indices
// that the group loaded at once is whole blocks.  Every lane of the group passes the same (b, n): the body may shuffle in the group.
template <bool HASE, int GH, class Body>
__device__ __forceinline__ void for_blocks(const Args &a, const Lane<GH> &ln, int64_t b, int64_t n, Body body)
{
    for (int64_t w0 = 0; w0 < n; w0 += a.GE) {
        const int64_t q = w0 + ln.li;
        const int64_t p = b + (q < n ? q : n - 1);
        const int32_t myc = a.colidx[p];
        int32_t mye = 0;
        if constexpr (HASE) mye = a.eidx ? a.eidx[p] : (int32_t)p;
        const int left = n - w0 < a.GE ? (int)(n - w0) : a.GE;
        for (int k = 0; k < left; k += kBlock) {
            const int cnt = left - k < kBlock ? left - k : kBlock;
            int32_t c[kBlock], e[kBlock];
#pragma unroll
            for (int u = 0; u < kBlock; u++) {
                const int src = ln.gbase + k + (u < cnt ? u : cnt - 1);
                c[u] = __shfl(myc, src, 64);
                e[u] = HASE ? __shfl(mye, src, 64) : 0;
            }
            body(cnt, c, e);
        }
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
// the online softmax over the entries b .. b + n - 1 (a row or a segment), continuing (m, z, N)
template <int GH, bool VEC, bool HASE>
__device__ __forceinline__ void fwd_entries(const Args &a, const Lane<GH> &ln, int64_t b, int64_t n, const float4 &q, float &m, float &z, float4 &N)
{
    for_blocks<HASE>(a, ln, b, n, [&](int cnt, const int32_t *c, const int32_t *e) {
        float4 k[kBlock], v[kBlock], ed[kBlock];
#pragma unroll
        for (int u = 0; u < kBlock; u++) {   // 12 loads requested before the first is consumed
            k[u] = ln.template load<VEC>(a.K + (int64_t)c[u] * a.ldk);
            if constexpr (HASE) ed[u] = ln.template load<VEC>(a.E + (int64_t)e[u] * a.lde);
            v[u] = ln.template load<VEC>(a.V + (int64_t)c[u] * a.ldv);
        }
        float s[kBlock];
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            if constexpr (HASE) k[u] = add4(k[u], ed[u]), v[u] = add4(v[u], ed[u]);
            s[u] = ln.template partial<VEC>(q, k[u]);
        }
        butterflies<GH>(s);
        float m_new = m;
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            s[u] = u < cnt ? a.scale * s[u] : -INFINITY;
            m_new = fmaxf(m_new, s[u]);
        }
        const float r = rescale_of(m, m_new);
        z = z * r;
        N = mul4(N, r);
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            if (u < cnt) {
                const float x = expf(s[u] - m_new);
                z = z + x;
                N = mul_add(N, v[u], x);
            }
        }
        m = m_new;
    });
}

// grid.x: blocks of 256 / GE rows; grid.y: passes of HP heads
template <int GH, bool VEC, bool HASE>
__global__ __launch_bounds__(256) void fwd_rows_kernel(Args a)
{
    const Lane<GH> ln(a);
    const int64_t row = group_index(a);
    if (row >= a.n_rows) return;   // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int64_t b = a.rowptr[row];
    int64_t d = (int64_t)a.rowptr[row + 1] - b;
    d = d < 0 ? 0 : d;
    if (d > kSeg) {
        if (blockIdx.y == 0 && ln.li == 0 && a.w.hubs.cap_hub > 0) append(a.w.hubs, (int32_t)row, d);
        return;
    }
    const float4 q = ln.template load<VEC>(a.Q + row * a.ldq);
    float m = -INFINITY, z = 0.f;
    float4 N = zero4();
    fwd_entries<GH, VEC, HASE>(a, ln, b, d, q, m, z, N);
    ln.template store<VEC>(a.A + row * a.lda, d == 0 ? zero4() : div4(N, z));
    if (ln.first) {
        if (a.rowmax_out) a.rowmax_out[row * a.H + ln.h] = m;   // an empty row: -inf
        if (a.rowsum_out) a.rowsum_out[row * a.H + ln.h] = z;   //               +0
    }
}

// (m_s, z_s, N_s) of every segment -> part_h, part_f
template <int GH, bool VEC, bool HASE>
__global__ __launch_bounds__(256) void fwd_seg_kernel(Args a)
{
    const Lane<GH> ln(a);
    const int64_t F = (int64_t)a.H * a.D;
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        const float4 q = ln.template load<VEC>(a.Q + (int64_t)row * a.ldq);
        float m = -INFINITY, z = 0.f;
        float4 N = zero4();
        fwd_entries<GH, VEC, HASE>(a, ln, b, n, q, m, z, N);
        ln.template store<VEC>(a.w.part_f + slot * 2 * F, N);
        if (ln.first) {
            a.w.part_h[slot * 2 * a.H + ln.h] = m;
            a.w.part_h[slot * 2 * a.H + a.H + ln.h] = z;
        }
    });
}

// A thread per (hub, element): the slots' partial results combined in ascending segment order, then the call's epilogue.
//   MODE 0 (forward): m = max m_s, z = sum z_s w_s, Y = (sum N_s w_s) / z;  MODE 1 (row side): dQ = scale * sum;
//   MODE 2 (column side): dV (+)= sum of the first partial, dK (+)= scale * sum of the second
template <int MODE>
__global__ __launch_bounds__(256) void hub_combine_kernel(Args a)
{
    const int64_t F = (int64_t)a.H * a.D;
    const int64_t total = listed_hubs(a.w.hubs) * F;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t hub = idx / F;
        const int64_t f = idx - hub * F;
        const int32_t h = (int32_t)(f / a.D);
        const int32_t row = a.w.hubs.hub_rows[hub];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t s0 = a.w.hubs.hub_seg0[hub];
        const float *pf = a.w.part_f + s0 * 2 * F + f;
        if constexpr (MODE == 0) {
            const float *pm = a.w.part_h + s0 * 2 * a.H + h, *pz = pm + a.H;
            float m = pm[0];
            for (int64_t s = 1; s < nseg; s++) m = fmaxf(m, pm[s * 2 * a.H]);
            float w = rescale_of(pm[0], m);
            float z = pz[0] * w, N = pf[0] * w;
            for (int64_t s = 1; s < nseg; s++) {
                w = rescale_of(pm[s * 2 * a.H], m);
                z = z + (pz[s * 2 * a.H] * w);
                N = N + (pf[s * 2 * F] * w);
            }
            a.A[(int64_t)row * a.lda + f] = __fdiv_rn(N, z);
            if (f == (int64_t)h * a.D) {
                if (a.rowmax_out) a.rowmax_out[(int64_t)row * a.H + h] = m;
                if (a.rowsum_out) a.rowsum_out[(int64_t)row * a.H + h] = z;
            }
        } else {
            float sa = pf[0], sb = MODE == 2 ? pf[F] : 0.f;
            for (int64_t s = 1; s < nseg; s++) {
                sa = sa + pf[s * 2 * F];
                if constexpr (MODE == 2) sb = sb + pf[s * 2 * F + F];
            }
            float *da = a.A + (int64_t)row * a.lda + f;
            if constexpr (MODE == 1) {
                *da = a.scale * sa;
            } else {
                float *db = a.B + (int64_t)row * a.ldb + f;
                sb = a.scale * sb;
                *da = a.beta ? *da + sa : sa;
                *db = a.beta ? *db + sb : sb;
            }
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// row side: dq += ds_p k'_p over the entries b .. b + n - 1 of row i, whose Q and G chunks are q and g; writes the entries' dE rows
template <int GH, bool VEC, bool HASE>
__device__ __forceinline__ void rows_entries(const Args &a, const Lane<GH> &ln, int64_t b, int64_t n, const float4 &q, const float4 &g, float m,
                                             float z, float dot, float4 &dq)
{
    for_blocks<HASE>(a, ln, b, n, [&](int cnt, const int32_t *c, const int32_t *e) {
        float4 k[kBlock], v[kBlock], ed[kBlock];
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            k[u] = ln.template load<VEC>(a.K + (int64_t)c[u] * a.ldk);
            if constexpr (HASE) ed[u] = ln.template load<VEC>(a.E + (int64_t)e[u] * a.lde);
            v[u] = ln.template load<VEC>(a.V + (int64_t)c[u] * a.ldv);
        }
        float t[2 * kBlock];   // s, then dalpha
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            if constexpr (HASE) k[u] = add4(k[u], ed[u]), v[u] = add4(v[u], ed[u]);
            t[u] = ln.template partial<VEC>(q, k[u]);
            t[kBlock + u] = ln.template partial<VEC>(g, v[u]);
        }
        butterflies<GH>(t);
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            if (u < cnt) {
                const float al = __fdiv_rn(expf(a.scale * t[u] - m), z);
                const float ds = al * (t[kBlock + u] - dot);
                dq = mul_add(dq, k[u], ds);
                if constexpr (HASE) ln.template store<VEC>(a.dE + (int64_t)e[u] * a.ldde, add4(mul4(g, al), mul4(q, a.scale * ds)));
            }
        }
    });
}

template <int GH, bool VEC, bool HASE>
__global__ __launch_bounds__(256) void bwd_rows_kernel(Args a)
{
    const Lane<GH> ln(a);
    const int64_t row = group_index(a);
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row];
    int64_t d = (int64_t)a.rowptr[row + 1] - b;
    d = d < 0 ? 0 : d;
    const float4 g = ln.template load<VEC>(a.G + row * a.ldg);
    float dot[1] = {ln.template partial<VEC>(g, ln.template load<VEC>(a.Yin + row * a.ldyin))};
    butterflies<GH>(dot);
    if (ln.first) a.dot_out[row * a.H + ln.h] = dot[0];
    if (d > kSeg) {   // the segment kernel reads dot back
        if (blockIdx.y == 0 && ln.li == 0 && a.w.hubs.cap_hub > 0) append(a.w.hubs, (int32_t)row, d);
        return;
    }
    const float4 q = ln.template load<VEC>(a.Q + row * a.ldq);
    float4 dq = zero4();
    if (d > 0) rows_entries<GH, VEC, HASE>(a, ln, b, d, q, g, a.rowmax[row * a.H + ln.hs], a.rowsum[row * a.H + ln.hs], dot[0], dq);
    ln.template store<VEC>(a.A + row * a.lda, mul4(dq, a.scale));   // an empty row: scale * +0
}

template <int GH, bool VEC, bool HASE>
__global__ __launch_bounds__(256) void bwd_rows_seg_kernel(Args a)
{
    const Lane<GH> ln(a);
    const int64_t F = (int64_t)a.H * a.D;
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        const float4 q = ln.template load<VEC>(a.Q + (int64_t)row * a.ldq);
        const float4 g = ln.template load<VEC>(a.G + (int64_t)row * a.ldg);
        const int64_t at = (int64_t)row * a.H + ln.hs;
        float4 dq = zero4();
        rows_entries<GH, VEC, HASE>(a, ln, b, n, q, g, a.rowmax[at], a.rowsum[at], a.dot_out[at], dq);
        ln.template store<VEC>(a.w.part_f + slot * 2 * F, dq);
    });
}

// column side, on the transposed pattern: row c with its own K and V chunks ko, vo; the entries are the rows i of the forward.
// dv += alpha_ic G_i;  dk += ds_ic Q_i
template <int GH, bool VEC, bool HASE>
__device__ __forceinline__ void cols_entries(const Args &a, const Lane<GH> &ln, int64_t b, int64_t n, const float4 &ko, const float4 &vo, float4 &dv,
                                             float4 &dk)
{
    for_blocks<HASE>(a, ln, b, n, [&](int cnt, const int32_t *c, const int32_t *e) {
        float m[kBlock], z[kBlock], dot[kBlock];
        float4 q[kBlock], g[kBlock], ed[kBlock];
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            const int64_t at = (int64_t)c[u] * a.H + ln.hs;
            m[u] = a.rowmax[at];
            z[u] = a.rowsum[at];
            dot[u] = a.dot[at];
            q[u] = ln.template load<VEC>(a.Q + (int64_t)c[u] * a.ldq);
            if constexpr (HASE) ed[u] = ln.template load<VEC>(a.E + (int64_t)e[u] * a.lde);
            g[u] = ln.template load<VEC>(a.G + (int64_t)c[u] * a.ldg);
        }
        float t[2 * kBlock];   // s, then dalpha
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            float4 k = ko, v = vo;
            if constexpr (HASE) k = add4(ko, ed[u]), v = add4(vo, ed[u]);
            t[u] = ln.template partial<VEC>(q[u], k);
            t[kBlock + u] = ln.template partial<VEC>(g[u], v);
        }
        butterflies<GH>(t);
#pragma unroll
        for (int u = 0; u < kBlock; u++) {
            if (u < cnt) {
                const float al = __fdiv_rn(expf(a.scale * t[u] - m[u]), z[u]);
                const float ds = al * (t[kBlock + u] - dot[u]);
                dv = mul_add(dv, g[u], al);
                dk = mul_add(dk, q[u], ds);
            }
        }
    });
}

template <int GH, bool VEC, bool HASE>
__global__ __launch_bounds__(256) void bwd_cols_kernel(Args a)
{
    const Lane<GH> ln(a);
    const int64_t row = group_index(a);
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row];
    int64_t d = (int64_t)a.rowptr[row + 1] - b;
    d = d < 0 ? 0 : d;
    if (d > kSeg) {
        if (blockIdx.y == 0 && ln.li == 0 && a.w.hubs.cap_hub > 0) append(a.w.hubs, (int32_t)row, d);
        return;
    }
    const float4 ko = ln.template load<VEC>(a.K + row * a.ldk), vo = ln.template load<VEC>(a.V + row * a.ldv);
    float4 dv = zero4(), dk = zero4();
    if (d > 0) cols_entries<GH, VEC, HASE>(a, ln, b, d, ko, vo, dv, dk);
    dk = mul4(dk, a.scale);
    float *pv = a.A + row * a.lda, *pk = a.B + row * a.ldb;
    if (a.beta) {
        dv = add4(ln.template load<VEC>(pv), dv);
        dk = add4(ln.template load<VEC>(pk), dk);
    }
    ln.template store<VEC>(pv, dv);
    ln.template store<VEC>(pk, dk);
}

template <int GH, bool VEC, bool HASE>
__global__ __launch_bounds__(256) void bwd_cols_seg_kernel(Args a)
{
    const Lane<GH> ln(a);
    const int64_t F = (int64_t)a.H * a.D;
    for_hub_segments(a.w.hubs, a.rowptr, group_index(a), group_count(a), [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        const float4 ko = ln.template load<VEC>(a.K + (int64_t)row * a.ldk), vo = ln.template load<VEC>(a.V + (int64_t)row * a.ldv);
        float4 dv = zero4(), dk = zero4();
        cols_entries<GH, VEC, HASE>(a, ln, b, n, ko, vo, dv, dk);
        ln.template store<VEC>(a.w.part_f + slot * 2 * F, dv);
        ln.template store<VEC>(a.w.part_f + slot * 2 * F + F, dk);
    });
}

// the two counter words, cleared by a kernel (not a memset node: the call may be recorded into a graph)
__global__ void zero_counters_kernel(int32_t *counters)
{
    if (threadIdx.x < kCounters) counters[threadIdx.x] = 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Shape {
    int GH, GE, HP;
    int64_t passes;
};

Shape shape_of(int32_t H, int32_t D)
{
    Shape s{};
    const int64_t Q = ((int64_t)D + 3) / 4;
    s.GH = 1;
    while (s.GH < Q && s.GH < 64) s.GH <<= 1;
    s.GE = s.GH < kBlock ? kBlock : s.GH;
    while (s.GE < 64 && s.GE < (int64_t)s.GH * H) s.GE <<= 1;
    s.HP = s.GE / s.GH;
    s.passes = ceil_div(H, s.HP);
    return s;
}

struct Sizes {
    int32_t n_rows, n_cols;
    int64_t nnz;
    const int32_t *rowptr, *colidx, *eidx;
    int64_t n_edge_rows;
    int32_t H, D;
    const float *E;
};

// what all three calls check before any HIP call
int check_common(const Sizes &z, Shape *s)
{
    GNNX_REQUIRE(z.n_rows >= 0 && z.n_cols >= 0 && z.nnz >= 0 && z.n_edge_rows >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(z.nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(z.H >= 1 && z.D >= 1, GNNX_ERR_INVALID_ARG, "n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE(z.nnz == 0 || (z.n_rows > 0 && z.n_cols > 0), GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    GNNX_REQUIRE(z.rowptr && (z.nnz == 0 || z.colidx), GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(z.E || !z.eidx, GNNX_ERR_INVALID_ARG, "edge indices without edge rows");
    GNNX_REQUIRE(!z.E || z.eidx || z.n_edge_rows >= z.nnz, GNNX_ERR_INVALID_ARG, "n_edge_rows < nnz without edge indices");
    GNNX_REQUIRE(z.D <= kMaxDim, GNNX_ERR_UNSUPPORTED, "head_dim %d > %d", z.D, kMaxDim);
    *s = shape_of(z.H, z.D);
    GNNX_REQUIRE(s->passes < 65536 && (int64_t)z.H * z.D + z.H < (1ll << 30), GNNX_ERR_UNSUPPORTED, "%d heads of %d features are too many for one launch",
                 z.H, z.D);
    return GNNX_OK;
}

int take_workspace(const Sizes &z, void *d_workspace, size_t workspace_bytes, Work *w)
{
    const size_t need = 256 + carve(z.n_rows, z.nnz, z.H, (int64_t)z.H * z.D, nullptr, nullptr);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    carve(z.n_rows, z.nnz, z.H, (int64_t)z.H * z.D, d_workspace, w);
    return GNNX_OK;
}

dim3 rows_grid(int32_t n_rows, const Shape &s) { return dim3((uint32_t)ceil_div(n_rows, 256 / s.GE), (uint32_t)s.passes); }
dim3 seg_grid(const Work &w, const Shape &s)
{
    const int64_t groups = w.hubs.cap_seg < kSegGroups ? w.hubs.cap_seg : kSegGroups;
    return dim3((uint32_t)ceil_div(groups * s.GE, 256), (uint32_t)s.passes);
}
dim3 flat_grid(int64_t threads) { return dim3((uint32_t)ceil_div(threads < (1 << 24) ? threads : (1 << 24), 256)); }

// f(Int<GH>, bool_constant<VEC>, bool_constant<HASE>) for the runtime shape
template <class F>
void with_shape(const Shape &s, bool vec, bool has_e, F f)
{
    auto go = [&](auto gh) {
        if (vec) has_e ? f(gh, std::true_type{}, std::true_type{}) : f(gh, std::true_type{}, std::false_type{});
        else has_e ? f(gh, std::false_type{}, std::true_type{}) : f(gh, std::false_type{}, std::false_type{});
    };
    switch (s.GH) {
    case 1: return go(Int<1>{});
    case 2: return go(Int<2>{});
    case 4: return go(Int<4>{});
    case 8: return go(Int<8>{});
    case 16: return go(Int<16>{});
    case 32: return go(Int<32>{});
    default: return go(Int<64>{});
    }
}

#define ATTN_LAUNCH(kernel, grid) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a)
#define ATTN_KERNEL(name) (name<decltype(gh)::value, decltype(v)::value, decltype(he)::value>)

bool vec4(int64_t ld, const void *p) { return ld % 4 == 0 && aligned16(p); }

}  // namespace

GNNX_API int gnnx_attn_workspace(int32_t n_rows, int64_t nnz, int32_t n_heads, int32_t head_dim, size_t *workspace_bytes)
{
    GNNX_REQUIRE(workspace_bytes, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(n_rows >= 0 && nnz >= 0 && n_heads >= 1 && head_dim >= 1, GNNX_ERR_INVALID_ARG, "negative size, n_heads < 1 or head_dim < 1");
    GNNX_REQUIRE((int64_t)n_heads * head_dim + n_heads < (1ll << 30), GNNX_ERR_UNSUPPORTED, "%d heads of %d features are too many", n_heads, head_dim);
    *workspace_bytes = 256 + carve(n_rows, nnz, n_heads, (int64_t)n_heads * head_dim, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_attn_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_eidx,
                               int64_t n_edge_rows, int32_t n_heads, int32_t head_dim, float scale, const float *d_Q, int64_t ldq, const float *d_K,
                               int64_t ldk, const float *d_V, int64_t ldv, const float *d_E, int64_t lde, float *d_Y, int64_t ldy, float *d_rowmax,
                               float *d_rowsum, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const Sizes z{n_rows, n_cols, nnz, d_rowptr, d_colidx, d_eidx, n_edge_rows, n_heads, head_dim, d_E};
    Shape s;
    int rc = check_common(z, &s);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldq >= F && ldk >= F && ldv >= F && ldy >= F && (!d_E || lde >= F), GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(d_Q && d_Y && (nnz == 0 || (d_K && d_V)), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Args a{};
    rc = take_workspace(z, d_workspace, workspace_bytes, &a.w);
    if (rc) return rc;
    a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.rowptr = d_rowptr, a.colidx = d_colidx, a.eidx = d_eidx, a.scale = scale;
    a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.E = d_E, a.lde = lde, a.A = d_Y, a.lda = ldy;
    a.rowmax_out = d_rowmax, a.rowsum_out = d_rowsum, a.GE = s.GE, a.HP = s.HP;
    const bool vec = head_dim % 4 == 0 && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(lde, d_E) && vec4(ldy, d_Y);
    const bool hubs = a.w.hubs.cap_hub > 0;
    hipStream_t st = as_stream(stream);
    if (hubs) hipLaunchKernelGGL(zero_counters_kernel, dim3(1), dim3(64), 0, st, a.w.counters);
    with_shape(s, vec, d_E != nullptr, [&](auto gh, auto v, auto he) {
        ATTN_LAUNCH(ATTN_KERNEL(fwd_rows_kernel), rows_grid(n_rows, s));
        if (!hubs) return;
        ATTN_LAUNCH(ATTN_KERNEL(fwd_seg_kernel), seg_grid(a.w, s));
        ATTN_LAUNCH(hub_combine_kernel<0>, flat_grid(a.w.hubs.cap_hub * F));
    });
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_attn_bwd_rows_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                        const int32_t *d_eidx, int64_t n_edge_rows, int32_t n_heads, int32_t head_dim, float scale, const float *d_G,
                                        int64_t ldg, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
                                        const float *d_E, int64_t lde, const float *d_Y, int64_t ldy, const float *d_rowmax, const float *d_rowsum,
                                        float *d_dQ, int64_t lddq, float *d_dot, float *d_dE, int64_t ldde, void *d_workspace, size_t workspace_bytes,
                                        void *stream)
{
    const Sizes z{n_rows, n_cols, nnz, d_rowptr, d_colidx, d_eidx, n_edge_rows, n_heads, head_dim, d_E};
    Shape s;
    int rc = check_common(z, &s);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && ldy >= F && lddq >= F && (!d_E || (lde >= F && ldde >= F)), GNNX_ERR_INVALID_ARG,
                 "ld < n_heads * head_dim");
    GNNX_REQUIRE(d_G && d_Q && d_Y && d_rowmax && d_rowsum && d_dQ && d_dot && (nnz == 0 || (d_K && d_V)) && (!d_E || d_dE || nnz == 0),
                 GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Args a{};
    rc = take_workspace(z, d_workspace, workspace_bytes, &a.w);
    if (rc) return rc;
    a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.rowptr = d_rowptr, a.colidx = d_colidx, a.eidx = d_eidx, a.scale = scale;
    a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.E = d_E, a.lde = lde, a.G = d_G, a.ldg = ldg;
    a.Yin = d_Y, a.ldyin = ldy, a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot_out = d_dot, a.A = d_dQ, a.lda = lddq, a.dE = d_dE, a.ldde = ldde;
    a.GE = s.GE, a.HP = s.HP;
    const bool vec = head_dim % 4 == 0 && vec4(ldg, d_G) && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(lde, d_E) && vec4(ldy, d_Y) &&
                     vec4(lddq, d_dQ) && vec4(ldde, d_dE);
    const bool hubs = a.w.hubs.cap_hub > 0;
    hipStream_t st = as_stream(stream);
    if (hubs) hipLaunchKernelGGL(zero_counters_kernel, dim3(1), dim3(64), 0, st, a.w.counters);
    with_shape(s, vec, d_E != nullptr, [&](auto gh, auto v, auto he) {
        ATTN_LAUNCH(ATTN_KERNEL(bwd_rows_kernel), rows_grid(n_rows, s));
        if (!hubs) return;
        ATTN_LAUNCH(ATTN_KERNEL(bwd_rows_seg_kernel), seg_grid(a.w, s));
        ATTN_LAUNCH(hub_combine_kernel<1>, flat_grid(a.w.hubs.cap_hub * F));
    });
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

GNNX_API int gnnx_attn_bwd_cols_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                        const int32_t *d_eidx, int64_t n_edge_rows, int32_t n_heads, int32_t head_dim, float scale, const float *d_G,
                                        int64_t ldg, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
                                        const float *d_E, int64_t lde, const float *d_rowmax, const float *d_rowsum, const float *d_dot, float beta,
                                        float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const Sizes z{n_rows, n_cols, nnz, d_rowptr, d_colidx, d_eidx, n_edge_rows, n_heads, head_dim, d_E};
    Shape s;
    int rc = check_common(z, &s);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && lddk >= F && lddv >= F && (!d_E || lde >= F), GNNX_ERR_INVALID_ARG,
                 "ld < n_heads * head_dim");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE(d_K && d_V && d_dK && d_dV && (nnz == 0 || (d_G && d_Q && d_rowmax && d_rowsum && d_dot)), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Args a{};
    rc = take_workspace(z, d_workspace, workspace_bytes, &a.w);
    if (rc) return rc;
    a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.rowptr = d_rowptr, a.colidx = d_colidx, a.eidx = d_eidx, a.scale = scale;
    a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.E = d_E, a.lde = lde, a.G = d_G, a.ldg = ldg;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot = d_dot, a.A = d_dV, a.lda = lddv, a.B = d_dK, a.ldb = lddk, a.beta = beta != 0.f;
    a.GE = s.GE, a.HP = s.HP;
    const bool vec = head_dim % 4 == 0 && vec4(ldg, d_G) && vec4(ldq, d_Q) && vec4(ldk, d_K) && vec4(ldv, d_V) && vec4(lde, d_E) && vec4(lddk, d_dK) &&
                     vec4(lddv, d_dV);
    const bool hubs = a.w.hubs.cap_hub > 0;
    hipStream_t st = as_stream(stream);
    if (hubs) hipLaunchKernelGGL(zero_counters_kernel, dim3(1), dim3(64), 0, st, a.w.counters);
    with_shape(s, vec, d_E != nullptr, [&](auto gh, auto v, auto he) {
        ATTN_LAUNCH(ATTN_KERNEL(bwd_cols_kernel), rows_grid(n_rows, s));
        if (!hubs) return;
        ATTN_LAUNCH(ATTN_KERNEL(bwd_cols_seg_kernel), seg_grid(a.w, s));
        ATTN_LAUNCH(hub_combine_kernel<2>, flat_grid(a.w.hubs.cap_hub * F));
    });
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}
