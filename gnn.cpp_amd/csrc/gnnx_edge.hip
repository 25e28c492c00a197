// Aggregation of messages that carry a feature vector per edge -- include/gnnx.h "edge features" (GINE and the OGB-mol family):
//   forward:   Y[i, f] = (beta ? Y[i, f] : nothing) + sum over the entries p of row i of act(X[c_p, f] + E[e_p, f])
//   backward:  dE[e_p, f] = (act is ReLU and X[c_p, f] + E[e_p, f] <= 0) ? +0 : G[i, f]
// with c_p = colidx[p] and e_p = eidx[p] (p itself without eidx).  dX is the forward on the transposed pattern over dE, without X.
// The sum has the header's order -- segments of S = 4096 entries, each ONE accumulator from +0 walking from the segment's last entry
// to its first, the segment sums added in ascending order -- so how rows, segments and features map to lanes is NOT in the result.
//
// The design.  The forward reads TWO rows of F floats per stored entry and writes one per ROW; nothing is reused between entries except
// through the caches (X rows, by whoever names the same column), so there is no LDS: a lane keeps its own 16 bytes of the row in
// registers and the only exchange, the G column / edge indices a group fetched with one coalesced load, is a shuffle.
//   * rows of d <= S entries: a lane group of G = 4 .. 64 lanes per row (the smallest that covers F / 4 pieces, several feature tiles
//     in grid.y past 64 lanes), 256 / G rows per workgroup.  Lane l loads the pattern of entry hi - 1 - l of the current window of G
//     entries; the group then takes them four at a time: 4 shuffles of (c, e), then the 4 X gathers AND the 4 E loads -- eight
//     independent 16-byte requests per lane -- before the first add, then add / ReLU / accumulate in descending position.
//   * hub rows, d > S: the row kernel lists them (gnnx_worklist.h), a fixed grid of lane groups strides over the segment slots and
//     writes each segment's sum to the workspace, a thread per (hub, feature) adds them in ascending order.  A hub column of the
//     transposed pattern (dX) takes the same path, so it spreads over the device like a hub row.
//   * dE: the same lane groups; the lane keeps its piece of G[i] in registers for the whole row (segment), recomputes the message of
//     four entries from eight loads and stores four selected pieces.  Hub rows go through the same list and segment grid (no
//     partials, no combine): their d * F stores spread over the device.
//   * without eidx the E rows of a row are consecutive: a pure stream that is read once, next to X rows that should stay in L2.  The E
//     load of that case can be issued non-temporal (GNNX_EDGE_STREAM_NT; DESIGN.md section 5.13 has both timings).
// n_feat % 4 != 0 or any pointer / leading dimension off 16 bytes: the same kernels with one float per lane, the same bits.
// Every launch is on the caller's stream and every ordering is a stream ordering; nothing is allocated or synchronised; no atomics on
// any value (two counter atomics per hub row; an atomicMax on an INDEX in gnnx_csr_entry_edges).
#include "gnnx_lanes.h"
#include "gnnx_worklist.h"

#pragma clang fp contract(off)

using namespace gnnx;

#ifndef GNNX_EDGE_STREAM_NT
#define GNNX_EDGE_STREAM_NT 1   // the product's choice for the E stream without eidx: 1 non-temporal, 0 plain (measured: DESIGN.md 5.13)
#endif

namespace {

constexpr int kCounters = 16;     // int32 words in front of the workspace: [0], [1] the hub list's
constexpr int kSegGroups = 8192;  // lane groups of the segment kernels (stride over the slots)

// the caller's workspace, carved
struct Lists {
    int32_t *counters;    // kCounters words, zeroed by the first kernel of every call
    float *part;          // [cap_seg, F] a segment's sum (forward)
    HubList hubs;
};

// bytes the carving takes from the first 256-byte boundary on of a workspace at any address
size_t carve(int32_t n_rows, int64_t nnz, int32_t F, void *ws, Lists *out)
{
    Lists w{};
    w.hubs.size(n_rows, nnz);
    Carver c(ws ? aligned_base(ws) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);   // 64 bytes: the partials stay 16-byte aligned (F % 4 == 0)
    w.part = c.take<float>((size_t)w.hubs.cap_seg * F, 4);
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
    int32_t n_rows, F;
    const int32_t *rowptr, *colidx, *eidx;   // eidx null: entry p reads E row p
    const float *X;                          // null: the message is the E row itself
    int64_t ldx;
    const float *E;
    int64_t lde;
    int relu, beta;
    float *Y;                                // forward: the output; backward: unused
    int64_t ldy;
    const float *G;                          // backward: the gradient of Y
    int64_t ldg;
    float *dE;
    int64_t ldde;
};

typedef float v4f __attribute__((ext_vector_type(4)));

template <bool NT> __device__ __forceinline__ float load_e(const float *p, float)
{
    return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT> __device__ __forceinline__ float4 load_e(const float *p, float4)
{
    if (NT) {
        const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const float4 *>(p);
}

// ReLU of the contract: NaN, -0 and every negative become +0
__device__ __forceinline__ float relu(float m) { return m > 0.f ? m : 0.f; }
__device__ __forceinline__ float4 relu(float4 m) { return make_float4(relu(m.x), relu(m.y), relu(m.z), relu(m.w)); }
// the gradient passes where the message was positive: a select, no rounding
__device__ __forceinline__ float pass(float m, float g) { return m > 0.f ? g : 0.f; }
__device__ __forceinline__ float4 pass(float4 m, float4 g) { return make_float4(pass(m.x, g.x), pass(m.y, g.y), pass(m.z, g.z), pass(m.w, g.w)); }

// the messages of B entries k .. k + B - 1 from the top of the group's current window, before the activation: all shuffles, then all
// loads of both matrices, then the adds
template <int VEC, int B, bool NT>
__device__ __forceinline__ void messages(typename Piece<VEC>::F (&m)[B], int32_t (&r)[B], int k, int32_t myc, int32_t mye, int gbase, int64_t fa,
                                         const Args &a)
{
    using V = typename Piece<VEC>::F;
    int32_t c[B];
    V x[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
        c[u] = __shfl(myc, gbase + k + u, 64);
        r[u] = __shfl(mye, gbase + k + u, 64);
    }
    if (a.X) {
#pragma unroll
        for (int u = 0; u < B; u++) x[u] = *reinterpret_cast<const V *>(a.X + (int64_t)c[u] * a.ldx + fa);
    }
#pragma unroll
    for (int u = 0; u < B; u++) m[u] = load_e<NT>(a.E + (int64_t)r[u] * a.lde + fa, V{});
    if (a.X) {
#pragma unroll
        for (int u = 0; u < B; u++) m[u] = add(x[u], m[u]);
    }
}

// The entries e - 1 down to b in windows of G.  body(k, n, myc, mye): the window holds n entries, lane l of the group carries the
// pattern of its l-th from the top; the body takes them in batches from k = 0.  Every lane of the group runs every shuffle.
template <int G, class Body>
__device__ __forceinline__ void for_windows(int64_t b, int64_t e, int li, const Args &a, Body body)
{
    for (int64_t hi = e; hi > b; hi -= G) {
        int64_t q = hi - 1 - li;
        q = q >= b ? q : b;
        const int32_t myc = a.colidx[q];
        const int32_t mye = a.eidx ? a.eidx[q] : (int32_t)q;
        body(hi - b < G ? (int)(hi - b) : G, myc, mye);
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
// one accumulator per feature over the entries e - 1 down to b
template <int G, int VEC, bool NT>
__device__ __forceinline__ void fwd_span(typename Piece<VEC>::F &acc, int64_t b, int64_t e, int li, int gbase, int64_t fa, const Args &a)
{
    using V = typename Piece<VEC>::F;
    for_windows<G>(b, e, li, a, [&](int n, int32_t myc, int32_t mye) {
        int k = 0;
        for (; k + 4 <= n; k += 4) {
            V m[4];
            int32_t r[4];
            messages<VEC, 4, NT>(m, r, k, myc, mye, gbase, fa, a);
#pragma unroll
            for (int u = 0; u < 4; u++) acc = add(acc, a.relu ? relu(m[u]) : m[u]);
        }
        for (; k < n; k++) {
            V m[1];
            int32_t r[1];
            messages<VEC, 1, NT>(m, r, k, myc, mye, gbase, fa, a);
            acc = add(acc, a.relu ? relu(m[0]) : m[0]);
        }
    });
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

// grid.x: blocks of 256 / G rows; grid.y: tiles of G * VEC features.  A row longer than S goes to the hub list (tile 0 lists it).
template <int G, int VEC, bool NT>
__global__ __launch_bounds__(256) void fwd_rows_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    const Lane<G, VEC> t(a.F);
    const int64_t row = t.unit;
    if (row >= a.n_rows) return;                // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (t.li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    V acc;
    clear(acc);
    fwd_span<G, VEC, NT>(acc, b, e, t.li, t.gbase, t.fa, a);
    if (!t.active) return;
    V *dst = reinterpret_cast<V *>(a.Y + row * a.ldy + t.f0);
    *dst = a.beta ? add(*dst, acc) : acc;
}

template <int G, int VEC, bool NT>
__global__ __launch_bounds__(256) void fwd_seg_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    const Lane<G, VEC> t(a.F);
    for_hub_segments(w.hubs, a.rowptr, t.unit, (int64_t)gridDim.x * t.GROUPS, [&](int32_t, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) {
        V acc;
        clear(acc);
        fwd_span<G, VEC, NT>(acc, b, b + n, t.li, t.gbase, t.fa, a);
        if (t.active) *reinterpret_cast<V *>(w.part + slot * a.F + t.f0) = acc;
    });
}

// a thread per (hub, feature): ((seg_0 + seg_1) + seg_2) + ...
__global__ __launch_bounds__(256) void fwd_combine_kernel(Args a, Lists w)
{
    const int64_t total = listed_hubs(w.hubs) * a.F;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t h = idx / a.F, f = idx - h * a.F;
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t at = (int64_t)w.hubs.hub_seg0[h] * a.F + f;
        float z = w.part[at];
        for (int64_t s = 1; s < nseg; s++) z = z + w.part[at + s * a.F];
        float *dst = a.Y + (int64_t)row * a.ldy + f;
        *dst = a.beta ? *dst + z : z;
    }
}

// ---- backward to the edge rows -------------------------------------------------------------------------------------------------
// dE of the entries b .. e - 1 of a row whose gradient piece is g
template <int G, int VEC>
__device__ __forceinline__ void bwd_span(typename Piece<VEC>::F g, int64_t b, int64_t e, const Lane<G, VEC> &t, const Args &a)
{
    using V = typename Piece<VEC>::F;
    for_windows<G>(b, e, t.li, a, [&](int n, int32_t myc, int32_t mye) {
        int k = 0;
        for (; k + 4 <= n; k += 4) {
            V m[4];
            int32_t r[4];
            if (a.relu) {
                messages<VEC, 4, false>(m, r, k, myc, mye, t.gbase, t.fa, a);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) r[u] = __shfl(mye, t.gbase + k + u, 64);
            }
            if (t.active) {
#pragma unroll
                for (int u = 0; u < 4; u++) *reinterpret_cast<V *>(a.dE + (int64_t)r[u] * a.ldde + t.f0) = a.relu ? pass(m[u], g) : g;
            }
        }
        for (; k < n; k++) {
            V m[1];
            int32_t r[1];
            if (a.relu) messages<VEC, 1, false>(m, r, k, myc, mye, t.gbase, t.fa, a);
            else r[0] = __shfl(mye, t.gbase + k, 64);
            if (t.active) *reinterpret_cast<V *>(a.dE + (int64_t)r[0] * a.ldde + t.f0) = a.relu ? pass(m[0], g) : g;
        }
    });
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void bwd_rows_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    const Lane<G, VEC> t(a.F);
    const int64_t row = t.unit;
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (t.li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    if (e == b) return;
    bwd_span<G, VEC>(*reinterpret_cast<const V *>(a.G + row * a.ldg + t.fa), b, e, t, a);
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void bwd_seg_kernel(Args a, Lists w)
{
    using V = typename Piece<VEC>::F;
    const Lane<G, VEC> t(a.F);
    for_hub_segments(w.hubs, a.rowptr, t.unit, (int64_t)gridDim.x * t.GROUPS, [&](int32_t row, int32_t, int64_t, int64_t b, int64_t n, int64_t) {
        bwd_span<G, VEC>(*reinterpret_cast<const V *>(a.G + (int64_t)row * a.ldg + t.fa), b, b + n, t, a);
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
inline uint32_t combine_blocks(const HubList &w, int32_t F) { return (uint32_t)ceil_div(w.cap_hub * F < (1 << 19) ? w.cap_hub * F : (1 << 19), 256); }

template <int G, int VEC, bool NT>
int launch_fwd_as(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    hipLaunchKernelGGL(clear_counters_kernel, dim3(1), dim3(64), 0, st, w.counters);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL((fwd_rows_kernel<G, VEC, NT>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), tiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((fwd_seg_kernel<G, VEC, NT>), dim3(seg_blocks(w.hubs, G), tiles), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(fwd_combine_kernel, dim3(combine_blocks(w.hubs, a.F)), dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}

template <int G, int VEC>
int launch_fwd(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st) { return launch_fwd_as<G, VEC, false>(a, w, tiles, st); }

#if GNNX_EDGE_STREAM_NT || defined(GNNX_EXPERIMENTS)
template <int G, int VEC>
int launch_fwd_nt(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st) { return launch_fwd_as<G, VEC, true>(a, w, tiles, st); }
#endif

template <int G, int VEC>
int launch_bwd(const Args &a, const Lists &w, uint32_t tiles, hipStream_t st)
{
    hipLaunchKernelGGL(clear_counters_kernel, dim3(1), dim3(64), 0, st, w.counters);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL((bwd_rows_kernel<G, VEC>), dim3((uint32_t)ceil_div(a.n_rows, 256 / G), tiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (w.hubs.cap_hub > 0) {
        hipLaunchKernelGGL((bwd_seg_kernel<G, VEC>), dim3(seg_blocks(w.hubs, G), tiles), dim3(256), 0, st, a, w);
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

int dispatch_fwd(const Shape &sh, const Args &a, const Lists &w, hipStream_t st) { GNNX_DISPATCH_SHAPE(launch_fwd, sh, a, w, sh.tiles, st) }
#if GNNX_EDGE_STREAM_NT || defined(GNNX_EXPERIMENTS)
int dispatch_fwd_nt(const Shape &sh, const Args &a, const Lists &w, hipStream_t st) { GNNX_DISPATCH_SHAPE(launch_fwd_nt, sh, a, w, sh.tiles, st) }
#endif
int dispatch_bwd(const Shape &sh, const Args &a, const Lists &w, hipStream_t st) { GNNX_DISPATCH_SHAPE(launch_bwd, sh, a, w, sh.tiles, st) }

// what every entry point checks before any device call
int check_sizes(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_feat >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    return GNNX_OK;
}

int check_edges(int msg, const int32_t *d_eidx, int64_t n_edge_rows, int64_t nnz)
{
    GNNX_REQUIRE(msg == GNNX_EDGE_MSG_ADD || msg == GNNX_EDGE_MSG_RELU, GNNX_ERR_INVALID_ARG, "msg %d is neither GNNX_EDGE_MSG_ADD nor GNNX_EDGE_MSG_RELU", msg);
    GNNX_REQUIRE(n_edge_rows >= 0 && (d_eidx || n_edge_rows >= nnz), GNNX_ERR_INVALID_ARG, "E has %lld rows for %lld entries without eidx",
                 (long long)n_edge_rows, (long long)nnz);
    return GNNX_OK;
}

// ---- entry -> edge ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void entry_edges_clear_kernel(const int32_t *__restrict__ rowptr, int32_t n_rows, int32_t *eidx, int32_t *missing)
{
    const int64_t nnz = rowptr[n_rows];
    if (blockIdx.x == 0 && threadIdx.x == 0) *missing = 0;
    if (!eidx) return;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * 256) eidx[p] = -1;
}

// a lane per edge: the position of dst in the strictly ascending row src; of the edges that name one entry the largest index stays
__global__ __launch_bounds__(256) void entry_edges_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                           const int32_t *__restrict__ src, const int32_t *__restrict__ dst, int32_t n_rows,
                                                           int64_t n_edges, int32_t *eidx, int32_t *missing)
{
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n_edges; x += (int64_t)gridDim.x * 256) {
        const int32_t r = src[x], c = dst[x];
        if (r == c) continue;                       // the build removes self loops
        int64_t found = -1;
        if (r >= 0 && r < n_rows && colidx && eidx) {
            int64_t lo = rowptr[r];
            const int64_t end = rowptr[r + 1];
            int64_t hi = end;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (colidx[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < end && colidx[lo] == c) found = lo;
        }
        if (found >= 0) atomicMax(&eidx[found], (int32_t)x);
        else atomicAdd(missing, 1);
    }
}

// The workspace both calls require is the neighbourhood reductions' (gnnx_spmm_csr_reduce_workspace): the carving above is the front of
// that unit's layout without the positions, so it always fits.
int place_lists(int32_t n_rows, int64_t nnz, int32_t n_feat, void *d_workspace, size_t workspace_bytes, Lists *w)
{
    size_t need = 0;
    int rc = gnnx_spmm_csr_reduce_workspace(n_rows, nnz, n_feat, &need);
    if (rc) return rc;
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    GNNX_REQUIRE(256 + carve(n_rows, nnz, n_feat, d_workspace, w) <= need, GNNX_ERR_WORKSPACE, "the edge lists do not fit the reduce workspace");
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_spmm_csr_edge_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                    const int32_t *d_eidx, int64_t n_edge_rows, const float *d_X, int64_t ldx, const float *d_E, int64_t lde,
                                    int msg, float beta, float *d_Y, int64_t ldy, void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows, n_cols, n_feat, nnz);
    if (rc) return rc;
    rc = check_edges(msg, d_eidx, n_edge_rows, nnz);
    if (rc) return rc;
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE((!d_X || ldx >= n_feat) && lde >= n_feat && ldy >= n_feat, GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (n_rows == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr && d_Y && (nnz == 0 || (d_colidx && d_E)), GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    rc = place_lists(n_rows, nnz, n_feat, d_workspace, workspace_bytes, &w);
    if (rc) return rc;
    const bool vec = n_feat % 4 == 0 && (!d_X || (ldx % 4 == 0 && aligned16(d_X))) && lde % 4 == 0 && ldy % 4 == 0 && aligned16(d_E) && aligned16(d_Y);
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    const Args a{n_rows, n_feat, d_rowptr, d_colidx, d_eidx, d_X, ldx, d_E, lde, msg == GNNX_EDGE_MSG_RELU, beta != 0.f, d_Y, ldy, nullptr, 0, nullptr, 0};
#if GNNX_EDGE_STREAM_NT || defined(GNNX_EXPERIMENTS)
    bool nt = GNNX_EDGE_STREAM_NT != 0;
    if (const char *s = experiment_env("GNNX_EDGE_E_LOAD")) nt = s[0] == 'n';   // "nt" / "plain"
    if (nt && !d_eidx) return dispatch_fwd_nt(sh, a, w, as_stream(stream));
#endif
    return dispatch_fwd(sh, a, w, as_stream(stream));
}

GNNX_API int gnnx_spmm_csr_edge_bwd_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr,
                                        const int32_t *d_colidx, const int32_t *d_eidx, int64_t n_edge_rows, const float *d_X, int64_t ldx,
                                        const float *d_E, int64_t lde, int msg, const float *d_G, int64_t ldg, float *d_dE, int64_t ldde,
                                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows, n_cols, n_feat, nnz);
    if (rc) return rc;
    rc = check_edges(msg, d_eidx, n_edge_rows, nnz);
    if (rc) return rc;
    const bool relu = msg == GNNX_EDGE_MSG_RELU;   // ADD never reads X or E
    GNNX_REQUIRE((!relu || ((!d_X || ldx >= n_feat) && lde >= n_feat)) && ldg >= n_feat && ldde >= n_feat, GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (n_rows == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr && (nnz == 0 || (d_colidx && d_G && d_dE && (!relu || d_E))), GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    rc = place_lists(n_rows, nnz, n_feat, d_workspace, workspace_bytes, &w);
    if (rc) return rc;
    if (nnz == 0) return GNNX_OK;
    const bool vec = n_feat % 4 == 0 && ldg % 4 == 0 && ldde % 4 == 0 && aligned16(d_G) && aligned16(d_dE) &&
                     (!relu || ((!d_X || (ldx % 4 == 0 && aligned16(d_X))) && lde % 4 == 0 && aligned16(d_E)));
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    const Args a{n_rows, n_feat, d_rowptr, d_colidx, d_eidx, relu ? d_X : nullptr, ldx, d_E, lde, relu, 0, nullptr, 0, d_G, ldg, d_dE, ldde};
    return dispatch_bwd(sh, a, w, as_stream(stream));
}

GNNX_API int gnnx_csr_entry_edges(int32_t n_rows, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_src, const int32_t *d_dst,
                                  int64_t n_edges, int32_t *d_eidx, int32_t *d_missing, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && n_edges >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_edges < (1ll << 31), GNNX_ERR_INVALID_ARG, "n_edges does not fit an int32 edge index");
    GNNX_REQUIRE(d_rowptr && d_missing && (n_edges == 0 || (d_src && d_dst)), GNNX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = as_stream(stream);
    // d_colidx / d_eidx may be null for a pattern without entries: the clear kernel then writes nothing and no edge finds a partner
    const int64_t lanes = n_edges > (int64_t)n_rows * 16 ? n_edges : (int64_t)n_rows * 16;
    const uint32_t blocks = (uint32_t)(ceil_div(lanes > 0 ? lanes : 1, 256) < 65536 ? ceil_div(lanes > 0 ? lanes : 1, 256) : 65536);
    hipLaunchKernelGGL(entry_edges_clear_kernel, dim3(blocks), dim3(256), 0, st, d_rowptr, n_rows, d_eidx, d_missing);
    GNNX_LAUNCH_CHECK();
    if (n_edges > 0) {
        hipLaunchKernelGGL(entry_edges_kernel, dim3(blocks), dim3(256), 0, st, d_rowptr, d_colidx, d_src, d_dst, n_rows, n_edges, d_eidx, d_missing);
        GNNX_LAUNCH_CHECK();
    }
    return GNNX_OK;
}
