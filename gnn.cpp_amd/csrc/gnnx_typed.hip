// Aggregation over edges that carry a RELATION TYPE -- include/gnnx.h "relation-typed aggregation" (R-GCN and the heterogeneous-graph
// layers built on it).  With t_p = etype[p], c_p = colidx[p], v_p = vals[p] (1 without vals), R types and B output slabs:
//   forward, basis mode:    M[i, b F + f] = sum over the entries p of row i of (C[t_p, b] * v_p) * X[c_p, f]
//   forward, one-hot mode:  M[i, t_p F + f] takes v_p * X[c_p, f]; the other slabs of the row are not touched by the entry
//   backward:               dX[j, f] (+)= sum over the entries q of row j of CSR(A^T) of  sum_b w_qb * dM[c_q, b F + f]
//   coefficient gradient:   D[p, b] = v_p * <dM[i_p, b F ..], X[c_p, ..]>   (the dot of gnnx_edge_dot.h)
// The sums have the header's order -- segments of S = 4096 entries, each ONE accumulator per output element from +0 walking from the
// segment's last entry to its first, the segment sums added in ascending order -- so how rows, slabs and features map to lanes is NOT
// in the result.
//
// The design.  The forward reads ONE row of F floats per stored entry and feeds it to B accumulators: the traffic is that of a plain
// aggregation, the arithmetic B times as much, and the output row is B times as wide.
//   * rows of d <= S entries: a lane group of G = 4 .. 64 lanes per row, one 16-byte piece of the F features per lane (feature tiles in
//     grid.y), 256 / G rows per workgroup.  A lane keeps a register tile of BT in {1, 2, 4, 8} slab accumulators of its piece; more
//     than 8 slabs run in tiles of 8 in grid.z (the last may be partial).  Lane l loads (c, t, v) of entry hi - 1 - l of the current
//     window of G entries; the group takes them four at a time: 12 shuffles, then the 4 X gathers before the first multiply.
//   * the coefficients of the tile, C[:, b0 .. b0 + BT), are staged once per workgroup in dynamic LDS as [R][BT]: per entry a lane reads
//     BT consecutive words at t * BT -- one address for the whole lane group, a broadcast.
//   * one-hot mode needs no table.  A tile pass gathers X only for the entries whose type falls in its tile (a branch that is uniform in
//     the lane group), so every X row is gathered once per feature tile however many slab tiles there are, and an entry adds to ONE
//     accumulator: there is no 0 * x, an inf of one relation never reaches another's slab.
//   * hub rows, d > S: the row kernel lists them (gnnx_worklist.h), a fixed grid of lane groups strides over the segment slots and
//     writes each segment's B F sums to the workspace, a thread per (hub, element) adds them in ascending order.
//   * backward: the same lane groups on the transposed pattern.  Per entry a lane gathers its piece of all B slabs of one dM row -- B
//     independent 16-byte loads, in tiles of 4, two entries at a time -- and continues the chain u = w_0 g_0, u = u + w_b g_b across
//     the tiles in registers.  The table is the whole [R][B] in LDS.  One-hot mode loads the one slab the entry names.
//   * coefficient gradient: a lane group of the dot's G = 1 .. 64 lanes per row keeps chunk l of up to 4 slabs of dM[i] in registers for
//     the whole row (segment), gathers each X[c_p] chunk once (four entries requested before the first product) and reduces the tile's
//     partials by butterfly.  Chunks l + G, .. of rows wider than 256 features are re-read from dM (the caches hold the row).
// n_feat % 4 != 0 or any pointer / leading dimension off 16 bytes: the same kernels with one float per lane, the same bits.
// Every launch is on the caller's stream and every ordering is a stream ordering; nothing is allocated or synchronised; no atomics on
// any value (two counter atomics per hub row).
#include "gnnx_edge_dot.h"
#include "gnnx_lanes.h"
#include "gnnx_worklist.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kCounters = 16;             // int32 words in front of the workspace: [0], [1] the hub list's
constexpr int kSegGroups = 8192;          // lane groups of the segment kernels (stride over the slots)
constexpr int kTile = 8;                  // slabs of the widest register tile; the tile stride of grid.z
// Slabs per pass of the backward (dM pieces of two entries in registers) and of the coefficient gradient (dM chunks of the row in
// registers).  8, the forward's tile, made the compiler move 23 .. 62 scalar registers to vector lanes in those kernels; 4 leaves none
// in the row kernels (measured both ways: DESIGN.md section 5.15).
#ifndef GNNX_TYPED_BWD_TILE
#define GNNX_TYPED_BWD_TILE 4
#endif
#ifndef GNNX_TYPED_DOT_TILE
#define GNNX_TYPED_DOT_TILE 4
#endif
constexpr int kBwdTile = GNNX_TYPED_BWD_TILE, kDotTile = GNNX_TYPED_DOT_TILE;
constexpr size_t kMaxTable = 64 * 1024;   // bytes of LDS a coefficient table may take (every basis kernel opts in for this much)

// the caller's workspace, carved (the layout of gnnx_edge.hip with rows of `width` floats)
struct Lists {
    int32_t *counters;    // kCounters words, zeroed by the first kernel of every call
    float *part;          // [cap_seg, width] a segment's sums
    HubList hubs;
};

size_t carve(int32_t n_rows, int64_t nnz, int64_t width, void *ws, Lists *out)
{
    Lists w{};
    w.hubs.size(n_rows, nnz);
    Carver c(ws ? aligned_base(ws) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);   // 64 bytes: the partials stay 16-byte aligned (width % 4 == 0)
    w.part = c.take<float>((size_t)w.hubs.cap_seg * width, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hubs.take_slots(c);
    if (out) *out = w;
    return c.bytes();
}

// a captured graph must not hold a memset node: the counters are cleared by a kernel
__global__ void clear_counters_kernel(int32_t *counters)
{
    if (threadIdx.x < kCounters) counters[threadIdx.x] = 0;
}

struct Args {
    int32_t n_rows, F, R, B;
    const int32_t *rowptr, *colidx, *etype;
    const float *vals;       // null: every v_p is 1 and is not multiplied
    const float *C;          // [R, B] row-major; null: one-hot mode (B == R)
    const float *X;          // the gathered matrix: X (forward, coefficient gradient), dM (backward)
    int64_t ldx;
    const float *G;          // coefficient gradient: dM, read by row
    int64_t ldg;
    float *Y;                // forward: M; backward: dX
    int64_t ldy;
    float *D;                // coefficient gradient: [nnz, B]
    int beta;
};

// what a lane carries of one stored entry
struct Entry {
    int32_t c, t;
    float v;
};

__device__ __forceinline__ Entry load_entry(const Args &a, int64_t q)
{
    return Entry{a.colidx[q], a.etype[q], a.vals ? a.vals[q] : 1.f};
}

__device__ __forceinline__ Entry hand(const Entry &my, int lane)
{
    return Entry{__shfl(my.c, lane, 64), __shfl(my.t, lane, 64), __shfl(my.v, lane, 64)};
}

// The entries e - 1 down to b in windows of G.  body(n, my): the window holds n entries, lane l of the group carries the l-th from the
// top; the body takes them in batches from k = 0.  Every lane of the group runs every shuffle.
template <int G, class Body>
__device__ __forceinline__ void for_windows(int64_t b, int64_t e, int li, const Args &a, Body body)
{
    for (int64_t hi = e; hi > b; hi -= G) {
        int64_t q = hi - 1 - li;
        q = q >= b ? q : b;
        body(hi - b < G ? (int)(hi - b) : G, load_entry(a, q));
    }
}

// what a lane of a lane-group kernel is: its place in the group, its features, its row (or first slot)
template <int G, int VEC>
struct Lane {
    static constexpr int GROUPS = 256 / G;
    int li, gbase;
    int64_t f0, fa, unit;
    bool active;
    __device__ __forceinline__ Lane(int32_t F)
    {
        li = threadIdx.x % G;
        gbase = (threadIdx.x & 63) - li;
        f0 = ((int64_t)blockIdx.y * G + li) * VEC;
        active = f0 < F;                 // VEC == 4: F % 4 == 0, so the whole piece is inside the row
        fa = active ? f0 : 0;            // lanes past the row read feature 0 and never store
        unit = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    }
};

// the tile's columns of C as [R][BT] (zero behind the last slab), or all of it as [R][B] (BT == 0), once per workgroup
template <int BT>
__device__ __forceinline__ void stage_table(float *tab, int32_t b0, const Args &a)
{
    const int32_t width = BT ? BT : a.B;
    for (int32_t idx = threadIdx.x; idx < a.R * width; idx += 256) {
        const int32_t r = idx / width, b = b0 + idx % width;
        tab[idx] = b < a.B ? a.C[(int64_t)r * a.B + b] : 0.f;
    }
    __syncthreads();
}

// the slab an entry names takes the new sum, every other accumulator of the tile keeps its bits
__device__ __forceinline__ float pick(bool take, float s, float old) { return take ? s : old; }
__device__ __forceinline__ float4 pick(bool take, float4 s, float4 old)
{
    return make_float4(take ? s.x : old.x, take ? s.y : old.y, take ? s.z : old.z, take ? s.w : old.w);
}

// w_pb: one rounding, none without vals
__device__ __forceinline__ float weight(float c, float v, bool have_vals) { return have_vals ? c * v : c; }

// ---- forward -------------------------------------------------------------------------------------------------------------------
// NB entries from position k of the window: all shuffles, then all gathers, then per entry (descending position) the BT products and adds
template <int VEC, int BT, bool ONEHOT, int NB>
__device__ __forceinline__ void fwd_batch(typename Piece<VEC>::F (&acc)[BT], int k, const Entry &my, int gbase, int64_t fa, int32_t b0,
                                          const float *tab, const Args &a)
{
    using V = typename Piece<VEC>::F;
    Entry en[NB];
    V x[NB];
#pragma unroll
    for (int u = 0; u < NB; u++) en[u] = hand(my, gbase + k + u);
#pragma unroll
    for (int u = 0; u < NB; u++) {
        if (!ONEHOT || (uint32_t)(en[u].t - b0) < (uint32_t)BT) x[u] = *reinterpret_cast<const V *>(a.X + (int64_t)en[u].c * a.ldx + fa);
        else clear(x[u]);               // another tile's entry: never added
    }
#pragma unroll
    for (int u = 0; u < NB; u++) {
        if (ONEHOT) {
            const V m = a.vals ? mul(x[u], en[u].v) : x[u];
            const int32_t own = en[u].t - b0;
#pragma unroll
            for (int j = 0; j < BT; j++) acc[j] = pick(own == j, add(acc[j], m), acc[j]);   // a select: the tile stays in registers
        } else {
            const float *crow = tab + (int64_t)en[u].t * BT;
#pragma unroll
            for (int j = 0; j < BT; j++) acc[j] = add(acc[j], mul(x[u], weight(crow[j], en[u].v, a.vals != nullptr)));
        }
    }
}

// BT accumulators per feature over the entries e - 1 down to b
template <int G, int VEC, int BT, bool ONEHOT>
__device__ __forceinline__ void fwd_span(typename Piece<VEC>::F (&acc)[BT], int64_t b, int64_t e, const Lane<G, VEC> &t, int32_t b0,
                                         const float *tab, const Args &a)
{
    for_windows<G>(b, e, t.li, a, [&](int n, const Entry &my) {
        int k = 0;
        for (; k + 4 <= n; k += 4) fwd_batch<VEC, BT, ONEHOT, 4>(acc, k, my, t.gbase, t.fa, b0, tab, a);
        for (; k < n; k++) fwd_batch<VEC, BT, ONEHOT, 1>(acc, k, my, t.gbase, t.fa, b0, tab, a);
    });
}

// the tile's slabs of a row of `ld` floats at dst: slab b0 + j at column (b0 + j) F
template <int VEC, int BT>
__device__ __forceinline__ void store_tile(float *dst, const typename Piece<VEC>::F (&acc)[BT], int32_t b0, int64_t f0, const Args &a)
{
    using V = typename Piece<VEC>::F;
#pragma unroll
    for (int j = 0; j < BT; j++)
        if (b0 + j < a.B) *reinterpret_cast<V *>(dst + (int64_t)(b0 + j) * a.F + f0) = acc[j];
}

// grid.x: blocks of 256 / G rows; grid.y: tiles of G * VEC features; grid.z: tiles of 8 slabs.  A row longer than S goes to the hub list
// (the first tile of both lists it).
template <int G, int VEC, int BT, bool ONEHOT>
__global__ __launch_bounds__(256) void fwd_rows_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    extern __shared__ float tab[];
    const int32_t b0 = blockIdx.z * kTile;
    if (!ONEHOT) stage_table<BT>(tab, b0, a);
    const Lane<G, VEC> t(a.F);
    const int64_t row = t.unit;
    if (row >= a.n_rows) return;                // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (t.li == 0 && blockIdx.y == 0 && blockIdx.z == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    V acc[BT];
#pragma unroll
    for (int j = 0; j < BT; j++) clear(acc[j]);
    fwd_span<G, VEC, BT, ONEHOT>(acc, b, e, t, b0, tab, a);
    if (t.active) store_tile<VEC, BT>(a.Y + row * a.ldy, acc, b0, t.f0, a);
}

template <int G, int VEC, int BT, bool ONEHOT>
__global__ __launch_bounds__(256) void fwd_seg_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    extern __shared__ float tab[];
    const int32_t b0 = blockIdx.z * kTile;
    if (!ONEHOT) stage_table<BT>(tab, b0, a);
    const Lane<G, VEC> t(a.F);
    const int64_t width = (int64_t)a.B * a.F;
    for_hub_segments(w.hubs, a.rowptr, t.unit, (int64_t)gridDim.x * t.GROUPS, [&](int32_t, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        V acc[BT];
#pragma unroll
        for (int j = 0; j < BT; j++) clear(acc[j]);
        fwd_span<G, VEC, BT, ONEHOT>(acc, b, b + n, t, b0, tab, a);
        if (t.active) store_tile<VEC, BT>(w.part + slot * width, acc, b0, t.f0, a);
    });
}

// a thread per (hub, element of the `width` floats a segment wrote): ((seg_0 + seg_1) + seg_2) + ...
__global__ __launch_bounds__(256) void combine_kernel(Args a, Lists w, int64_t width)
{
    const int64_t total = listed_hubs(w.hubs) * width;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t h = idx / width, f = idx - h * width;
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t at = (int64_t)w.hubs.hub_seg0[h] * width + f;
        float z = w.part[at];
        for (int64_t s = 1; s < nseg; s++) z = z + w.part[at + s * width];
        float *dst = a.Y + (int64_t)row * a.ldy + f;
        *dst = a.beta ? *dst + z : z;
    }
}

// ---- backward to X ---------------------------------------------------------------------------------------------------------------
// NB entries from position k of the window; a.X is dM.  Basis mode: per entry the chain over b ascending, continued across the tiles.
template <int VEC, bool ONEHOT, int NB>
__device__ __forceinline__ void bwd_batch(typename Piece<VEC>::F &acc, int k, const Entry &my, int gbase, int64_t fa, const float *tab, const Args &a)
{
    using V = typename Piece<VEC>::F;
    Entry en[NB];
    V u[NB];
#pragma unroll
    for (int e = 0; e < NB; e++) en[e] = hand(my, gbase + k + e);
    if (ONEHOT) {
#pragma unroll
        for (int e = 0; e < NB; e++) u[e] = *reinterpret_cast<const V *>(a.X + (int64_t)en[e].c * a.ldx + (int64_t)en[e].t * a.F + fa);
#pragma unroll
        for (int e = 0; e < NB; e++) acc = add(acc, a.vals ? mul(u[e], en[e].v) : u[e]);
        return;
    }
    for (int32_t b0 = 0; b0 < a.B; b0 += kBwdTile) {
        V g[NB][kBwdTile];
#pragma unroll
        for (int e = 0; e < NB; e++) {
            const float *src = a.X + (int64_t)en[e].c * a.ldx + (int64_t)b0 * a.F + fa;
#pragma unroll
            for (int j = 0; j < kBwdTile; j++)
                if (b0 + j < a.B) g[e][j] = *reinterpret_cast<const V *>(src + (int64_t)j * a.F);
        }
#pragma unroll
        for (int e = 0; e < NB; e++) {
            const float *crow = tab + (int64_t)en[e].t * a.B + b0;
#pragma unroll
            for (int j = 0; j < kBwdTile; j++) {
                if (b0 + j < a.B) {
                    const V p = mul(g[e][j], weight(crow[j], en[e].v, a.vals != nullptr));
                    u[e] = b0 + j == 0 ? p : add(u[e], p);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NB; e++) acc = add(acc, u[e]);
}

template <int G, int VEC, bool ONEHOT>
__device__ __forceinline__ void bwd_span(typename Piece<VEC>::F &acc, int64_t b, int64_t e, const Lane<G, VEC> &t, const float *tab, const Args &a)
{
    constexpr int NB = ONEHOT ? 4 : 2;          // basis mode has up to 2 x 4 loads in flight already
    for_windows<G>(b, e, t.li, a, [&](int n, const Entry &my) {
        int k = 0;
        for (; k + NB <= n; k += NB) bwd_batch<VEC, ONEHOT, NB>(acc, k, my, t.gbase, t.fa, tab, a);
        for (; k < n; k++) bwd_batch<VEC, ONEHOT, 1>(acc, k, my, t.gbase, t.fa, tab, a);
    });
}

template <int G, int VEC, bool ONEHOT>
__global__ __launch_bounds__(256) void bwd_rows_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    extern __shared__ float tab[];
    if (!ONEHOT) stage_table<0>(tab, 0, a);
    const Lane<G, VEC> t(a.F);
    const int64_t row = t.unit;
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (t.li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    V acc;
    clear(acc);
    bwd_span<G, VEC, ONEHOT>(acc, b, e, t, tab, a);
    if (!t.active) return;
    V *dst = reinterpret_cast<V *>(a.Y + row * a.ldy + t.f0);
    *dst = a.beta ? add(*dst, acc) : acc;
}

template <int G, int VEC, bool ONEHOT>
__global__ __launch_bounds__(256) void bwd_seg_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    extern __shared__ float tab[];
    if (!ONEHOT) stage_table<0>(tab, 0, a);
    const Lane<G, VEC> t(a.F);
    for_hub_segments(w.hubs, a.rowptr, t.unit, (int64_t)gridDim.x * t.GROUPS, [&](int32_t, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        V acc;
        clear(acc);
        bwd_span<G, VEC, ONEHOT>(acc, b, b + n, t, tab, a);
        if (t.active) *reinterpret_cast<V *>(w.part + slot * a.F + t.f0) = acc;
    });
}

// ---- coefficient gradient --------------------------------------------------------------------------------------------------------
// The entries b .. e - 1 of row `row`: D[p, b0 + j] for the tile's slabs.  g0[j]: chunk li of slab b0 + j of dM[row], kept by the caller.
template <int G, bool VEC>
__device__ __forceinline__ void cg_span(const float4 (&g0)[kDotTile], const float *grow, int64_t b, int64_t e, int li, int gbase, int32_t b0, const Args &a)
{
    const int32_t Q = (a.F + 3) / 4;
    const bool have = li < Q;
    for (int64_t lo = b; lo < e; lo += G) {
        const int64_t q = lo + li < e ? lo + li : e - 1;
        const Entry my = load_entry(a, q);
        const int n = e - lo < G ? (int)(e - lo) : G;
        for (int k = 0; k < n; k += kInFlight) {
            Entry en[kInFlight];
            float4 x[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; u++) en[u] = hand(my, gbase + (k + u < n ? k + u : n - 1));
#pragma unroll
            for (int u = 0; u < kInFlight; u++)
                x[u] = have ? load_chunk<VEC>(a.X + (int64_t)en[u].c * a.ldx, li, a.F) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                if (k + u >= n) break;              // uniform in the group
                float acc[kDotTile];
#pragma unroll
                for (int j = 0; j < kDotTile; j++) {
                    acc[j] = 0.f;
                    if (have && b0 + j < a.B) acc[j] = add_chunk<VEC>(acc[j], g0[j], x[u], li, a.F);
                }
                for (int32_t c = li + G; c < Q; c += G) {      // rows wider than 4 G features: the further chunks of the lane
                    const float4 xc = load_chunk<VEC>(a.X + (int64_t)en[u].c * a.ldx, c, a.F);
#pragma unroll
                    for (int j = 0; j < kDotTile; j++)
                        if (b0 + j < a.B) acc[j] = add_chunk<VEC>(acc[j], load_chunk<VEC>(grow + (int64_t)(b0 + j) * a.F, c, a.F), xc, c, a.F);
                }
#pragma unroll
                for (int j = 0; j < kDotTile; j++) {
                    if (b0 + j >= a.B) break;
                    const float d = butterfly<G>(acc[j]);           // every lane of the group holds the sum
                    if (li == (j & (G - 1))) a.D[(lo + k + u) * a.B + b0 + j] = a.vals ? d * en[u].v : d;
                }
            }
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void load_row_tile(float4 (&g0)[kDotTile], const float *grow, int li, int32_t b0, const Args &a)
{
#pragma unroll
    for (int j = 0; j < kDotTile; j++)
        g0[j] = (li < (a.F + 3) / 4 && b0 + j < a.B) ? load_chunk<VEC>(grow + (int64_t)(b0 + j) * a.F, li, a.F) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid.x: blocks of 256 / G rows; grid.y: tiles of kDotTile slabs
template <int G, bool VEC>
__global__ __launch_bounds__(256) void cg_rows_kernel(Args a, Lists w)
{
    const int li = threadIdx.x % G, gbase = (threadIdx.x & 63) - li;
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int32_t b0 = blockIdx.y * kDotTile;
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    if (e == b) return;
    const float *grow = a.G + row * a.ldg;
    float4 g0[kDotTile];
    load_row_tile<VEC>(g0, grow, li, b0, a);
    cg_span<G, VEC>(g0, grow, b, e, li, gbase, b0, a);
}

template <int G, bool VEC>
__global__ __launch_bounds__(256) void cg_seg_kernel(Args a, Lists w)
{
    const int li = threadIdx.x % G, gbase = (threadIdx.x & 63) - li;
    const int32_t b0 = blockIdx.y * kDotTile;
    for_hub_segments(w.hubs, a.rowptr, (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G, (int64_t)gridDim.x * (256 / G),
                     [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t) {
                         const float *grow = a.G + (int64_t)row * a.ldg;
                         float4 g0[kDotTile];
                         load_row_tile<VEC>(g0, grow, li, b0, a);
                         cg_span<G, VEC>(g0, grow, b, b + n, li, gbase, b0, a);
                     });
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
inline uint32_t combine_blocks(const HubList &w, int64_t width) { return (uint32_t)ceil_div(w.cap_hub * width < (1 << 19) ? w.cap_hub * width : (1 << 19), 256); }

// the table's bytes are opted in and checked once per kernel and device, for the largest table the entry points admit
template <class K>
int table_opt_in(K kernel, std::atomic<uint64_t> &done, const char *what) { return lds_opt_in(kernel, kMaxTable, done, what); }

template <int G, int VEC, int BT, bool ONEHOT>
int launch_fwd(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    const size_t lds = ONEHOT ? 0 : sizeof(float) * a.R * BT;
    if (!ONEHOT) {
        static std::atomic<uint64_t> done_rows{0}, done_seg{0};
        int rc = table_opt_in(&fwd_rows_kernel<G, VEC, BT, ONEHOT>, done_rows, "typed fwd_rows_kernel");
        if (rc == GNNX_OK) rc = table_opt_in(&fwd_seg_kernel<G, VEC, BT, ONEHOT>, done_seg, "typed fwd_seg_kernel");
        if (rc != GNNX_OK) return rc;
    }
    const uint32_t ztiles = (uint32_t)ceil_div(a.B, kTile);
    hipLaunchKernelGGL(clear_counters_kernel, dim3(1), dim3(64), 0, st, w.counters);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL((fwd_rows_kernel<G, VEC, BT, ONEHOT>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), tiles, ztiles), dim3(256), lds, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((fwd_seg_kernel<G, VEC, BT, ONEHOT>), dim3(seg_blocks(w.hubs, G), tiles, ztiles), dim3(256), lds, st, a, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(combine_kernel, dim3(combine_blocks(w.hubs, (int64_t)a.B * a.F)), dim3(256), 0, st, a, w, (int64_t)a.B * a.F);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

// the register tile: the smallest of 1, 2, 4, 8 that holds the slabs; 8 with several tiles in grid.z beyond
template <int G, int VEC, bool ONEHOT>
int launch_fwd_tile(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    if (a.B <= 1) return launch_fwd<G, VEC, 1, ONEHOT>(a, w, tiles, st);
    if (a.B <= 2) return launch_fwd<G, VEC, 2, ONEHOT>(a, w, tiles, st);
    if (a.B <= 4) return launch_fwd<G, VEC, 4, ONEHOT>(a, w, tiles, st);
    return launch_fwd<G, VEC, kTile, ONEHOT>(a, w, tiles, st);
}

template <int G, int VEC>
int launch_fwd_mode(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    return a.C ? launch_fwd_tile<G, VEC, false>(a, w, tiles, st) : launch_fwd_tile<G, VEC, true>(a, w, tiles, st);
}

template <int G, int VEC, bool ONEHOT>
int launch_bwd(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    const size_t lds = ONEHOT ? 0 : sizeof(float) * a.R * a.B;
    if (!ONEHOT) {
        static std::atomic<uint64_t> done_rows{0}, done_seg{0};
        int rc = table_opt_in(&bwd_rows_kernel<G, VEC, ONEHOT>, done_rows, "typed bwd_rows_kernel");
        if (rc == GNNX_OK) rc = table_opt_in(&bwd_seg_kernel<G, VEC, ONEHOT>, done_seg, "typed bwd_seg_kernel");
        if (rc != GNNX_OK) return rc;
    }
    hipLaunchKernelGGL(clear_counters_kernel, dim3(1), dim3(64), 0, st, w.counters);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL((bwd_rows_kernel<G, VEC, ONEHOT>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), tiles), dim3(256), lds, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((bwd_seg_kernel<G, VEC, ONEHOT>), dim3(seg_blocks(w.hubs, G), tiles), dim3(256), lds, st, a, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(combine_kernel, dim3(combine_blocks(w.hubs, a.F)), dim3(256), 0, st, a, w, (int64_t)a.F);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

template <int G, int VEC>
int launch_bwd_mode(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    return a.C ? launch_bwd<G, VEC, false>(a, w, tiles, st) : launch_bwd<G, VEC, true>(a, w, tiles, st);
}

#define GNNX_DISPATCH_SHAPE(LAUNCH, sh, ...)                                                         \
    switch ((sh).G) {                                                                                \
    case 4: return (sh).vec ? LAUNCH<4, 4>(__VA_ARGS__) : LAUNCH<4, 1>(__VA_ARGS__);                 \
    case 8: return (sh).vec ? LAUNCH<8, 4>(__VA_ARGS__) : LAUNCH<8, 1>(__VA_ARGS__);                 \
    case 16: return (sh).vec ? LAUNCH<16, 4>(__VA_ARGS__) : LAUNCH<16, 1>(__VA_ARGS__);              \
    case 32: return (sh).vec ? LAUNCH<32, 4>(__VA_ARGS__) : LAUNCH<32, 1>(__VA_ARGS__);              \
    default: return (sh).vec ? LAUNCH<64, 4>(__VA_ARGS__) : LAUNCH<64, 1>(__VA_ARGS__);              \
    }

int dispatch_fwd(const Shape &sh, const Args &a, const Lists &w, hipStream_t st) { GNNX_DISPATCH_SHAPE(launch_fwd_mode, sh, a, w, sh.tiles, st) }
int dispatch_bwd(const Shape &sh, const Args &a, const Lists &w, hipStream_t st) { GNNX_DISPATCH_SHAPE(launch_bwd_mode, sh, a, w, sh.tiles, st) }

template <int G, bool VEC>
int launch_cg(const Args &a, const Lists &w, hipStream_t st)
{
    const uint32_t ztiles = (uint32_t)ceil_div(a.B, kDotTile);
    hipLaunchKernelGGL(clear_counters_kernel, dim3(1), dim3(64), 0, st, w.counters);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL((cg_rows_kernel<G, VEC>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), ztiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((cg_seg_kernel<G, VEC>), dim3(seg_blocks(w.hubs, G), ztiles), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

// the dot's lane group (gnnx_edge_dot.h): the smallest power of two that covers the Q chunks, 64 at most
template <bool VEC>
int dispatch_cg(const Args &a, const Lists &w, hipStream_t st)
{
    const int32_t Q = (a.F + 3) / 4;
    if (Q <= 1) return launch_cg<1, VEC>(a, w, st);
    if (Q <= 2) return launch_cg<2, VEC>(a, w, st);
    if (Q <= 4) return launch_cg<4, VEC>(a, w, st);
    if (Q <= 8) return launch_cg<8, VEC>(a, w, st);
    if (Q <= 16) return launch_cg<16, VEC>(a, w, st);
    if (Q <= 32) return launch_cg<32, VEC>(a, w, st);
    return launch_cg<64, VEC>(a, w, st);
}

// what every entry point checks before any device call
int check_sizes(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, int32_t n_types, int32_t n_slabs, const float *d_C)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_feat >= 0 && nnz >= 0 && n_types >= 0 && n_slabs >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(nnz == 0 || (n_types > 0 && n_slabs > 0), GNNX_ERR_INVALID_ARG, "entries without relation types or output slabs");
    GNNX_REQUIRE(d_C || n_slabs == n_types, GNNX_ERR_INVALID_ARG, "one-hot mode (no coefficient table) needs n_slabs == n_types, got %d and %d",
                 n_slabs, n_types);
    GNNX_REQUIRE((int64_t)n_slabs * n_feat < (1ll << 31), GNNX_ERR_UNSUPPORTED, "n_slabs * n_feat does not fit an int32 width");
    GNNX_REQUIRE(ceil_div(n_slabs, kTile) < 65536, GNNX_ERR_UNSUPPORTED, "too many slabs for one launch");
    return GNNX_OK;
}

// The workspace every call requires is the neighbourhood reductions' (gnnx_spmm_csr_reduce_workspace) at the width of what a segment
// writes: the carving above is the front of that unit's layout, so it always fits.
int place_lists(int32_t n_rows, int64_t nnz, int64_t width, int64_t part_width, void *d_workspace, size_t workspace_bytes, Lists *w)
{
    size_t need = 0;
    int rc = gnnx_spmm_csr_reduce_workspace(n_rows, nnz, (int32_t)width, &need);
    if (rc) return rc;
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    GNNX_REQUIRE(256 + carve(n_rows, nnz, part_width, d_workspace, w) <= need, GNNX_ERR_WORKSPACE, "the typed lists do not fit the reduce workspace");
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_spmm_csr_typed_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, int32_t n_types, int32_t n_slabs,
                                     const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_etype, const float *d_vals,
                                     const float *d_C, const float *d_X, int64_t ldx, float *d_M, int64_t ldm, void *d_workspace,
                                     size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows, n_cols, n_feat, nnz, n_types, n_slabs, d_C);
    if (rc) return rc;
    const int64_t width = (int64_t)n_slabs * n_feat;
    GNNX_REQUIRE(ldx >= n_feat && ldm >= width, GNNX_ERR_INVALID_ARG, "ld < width");
    if (n_rows == 0 || width == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr && d_M && (nnz == 0 || (d_colidx && d_etype && d_X)), GNNX_ERR_INVALID_ARG, "null pointer");
    const int bt = n_slabs <= 1 ? 1 : n_slabs <= 2 ? 2 : n_slabs <= 4 ? 4 : kTile;
    GNNX_REQUIRE(!d_C || sizeof(float) * n_types * bt <= kMaxTable, GNNX_ERR_UNSUPPORTED, "a coefficient table of %d types does not fit %zu bytes of LDS",
                 n_types, kMaxTable);
    Lists w;
    rc = place_lists(n_rows, nnz, width, width, d_workspace, workspace_bytes, &w);
    if (rc) return rc;
    const bool vec = n_feat % 4 == 0 && ldx % 4 == 0 && ldm % 4 == 0 && aligned16(d_X) && aligned16(d_M);
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    const Args a{n_rows, n_feat, n_types, n_slabs, d_rowptr, d_colidx, d_etype, d_vals, d_C, d_X, ldx, nullptr, 0, d_M, ldm, nullptr, 0};
    return dispatch_fwd(sh, a, w, as_stream(stream));
}

GNNX_API int gnnx_spmm_csr_typed_bwd_f32(int32_t n_rows_t, int32_t n_cols_t, int32_t n_feat, int64_t nnz, int32_t n_types, int32_t n_slabs,
                                         const int32_t *d_rowptr_t, const int32_t *d_colidx_t, const int32_t *d_etype_t, const float *d_vals_t,
                                         const float *d_C, const float *d_dM, int64_t ldm, float beta, float *d_dX, int64_t lddx,
                                         void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows_t, n_cols_t, n_feat, nnz, n_types, n_slabs, d_C);
    if (rc) return rc;
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE(ldm >= (int64_t)n_slabs * n_feat && lddx >= n_feat, GNNX_ERR_INVALID_ARG, "ld < width");
    if (n_rows_t == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols_t > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr_t && d_dX && (nnz == 0 || (d_colidx_t && d_etype_t && d_dM)), GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(!d_C || sizeof(float) * n_types * n_slabs <= kMaxTable, GNNX_ERR_UNSUPPORTED,
                 "a coefficient table of %d x %d does not fit %zu bytes of LDS", n_types, n_slabs, kMaxTable);
    Lists w;
    rc = place_lists(n_rows_t, nnz, n_feat, n_feat, d_workspace, workspace_bytes, &w);
    if (rc) return rc;
    const bool vec = n_feat % 4 == 0 && ldm % 4 == 0 && lddx % 4 == 0 && aligned16(d_dM) && aligned16(d_dX);
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    const Args a{n_rows_t, n_feat, n_types, n_slabs, d_rowptr_t, d_colidx_t, d_etype_t, d_vals_t, d_C, d_dM, ldm, nullptr, 0, d_dX, lddx, nullptr,
                 beta != 0.f};
    return dispatch_bwd(sh, a, w, as_stream(stream));
}

GNNX_API int gnnx_typed_coeff_grad_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, int32_t n_types, int32_t n_slabs,
                                       const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_etype, const float *d_vals,
                                       const float *d_dM, int64_t ldm, const float *d_X, int64_t ldx, float *d_D, void *d_workspace,
                                       size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_feat >= 0 && nnz >= 0 && n_types >= 0 && n_slabs >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(nnz == 0 || (n_types > 0 && n_slabs > 0), GNNX_ERR_INVALID_ARG, "entries without relation types or output slabs");
    GNNX_REQUIRE((int64_t)n_slabs * n_feat < (1ll << 31), GNNX_ERR_UNSUPPORTED, "n_slabs * n_feat does not fit an int32 width");
    GNNX_REQUIRE(ceil_div(n_slabs, kDotTile) < 65536, GNNX_ERR_UNSUPPORTED, "too many slabs for one launch");
    GNNX_REQUIRE(ldm >= (int64_t)n_slabs * n_feat && ldx >= n_feat, GNNX_ERR_INVALID_ARG, "ld < width");
    if (n_rows == 0 || nnz == 0) return GNNX_OK;
    GNNX_REQUIRE(n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr && d_colidx && d_etype && d_D && (n_feat == 0 || (d_dM && d_X)), GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    const int rc = place_lists(n_rows, nnz, n_slabs, 0, d_workspace, workspace_bytes, &w);
    if (rc) return rc;
    const bool vec = n_feat % 4 == 0 && ldm % 4 == 0 && ldx % 4 == 0 && aligned16(d_dM) && aligned16(d_X);
    const Args a{n_rows, n_feat, n_types, n_slabs, d_rowptr, d_colidx, d_etype, d_vals, nullptr, d_X, ldx, d_dM, ldm, nullptr, 0, d_D, 0};
    return vec ? dispatch_cg<true>(a, w, as_stream(stream)) : dispatch_cg<false>(a, w, as_stream(stream));
}
