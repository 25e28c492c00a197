// Element-wise max / min over the stored entries of each CSR row, with its arg, and the backward that routes every gradient element
// to the entry that won -- include/gnnx.h "neighbourhood reductions".
//   forward:   t_p,f = vals[p] * X[c_p, f];  arg[i, f] = the FIRST position of row i that no entry beats;  Y[i, f] = t_arg,f
//   backward:  dX[c, f] = beta dX + sum over the entries q of row c of CSR(A^T) of (arg[i_q, f] == map_t[q] ? vals[map_t[q]] * G[i_q, f] : nothing)
// A maximum has no order, so the forward's bits are a function of the inputs alone; the backward's sum has the header's order: segments
// of S = 4096 entries, each ONE accumulator from +0 walking from the segment's last entry to its first, the segment sums added in
// ascending order.  How rows and segments map to lanes is NOT in the result:
//   * rows of d <= S entries: the lane-group shape of gnnx_heads.hip's aggregation -- G = 4 .. 64 lanes per row, lane l owns features
//     f0 .. f0 + VEC - 1 of tile blockIdx.y, the group fetches G entries of the pattern with one coalesced load and hands them out by
//     shuffle, four gathered rows are requested before the first is compared (added).  A lane carries (value, position) per feature;
//   * hub rows, d > S: the row kernel appends them to the hub list (gnnx_worklist.h), a fixed grid of lane groups strides over the
//     segment slots and writes each segment's (value, position) or sum to the workspace, and a thread per (hub, feature) finishes the
//     row: the better value wins and on equal values the smaller position (forward), ascending segment order (backward).
// MIN is MAX on the sign-flipped values: flipping the sign bit is exact both ways, keeps every tie a tie and the first of them first.
// The running value starts from the FIRST entry (position -1 means "none yet"), never from a sentinel: a row of -inf gets its first
// entry.  Every launch is on the caller's stream and every ordering is a stream ordering; nothing is allocated or synchronised.
#include "gnnx_lanes.h"
#include "gnnx_worklist.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kCounters = 16;     // int32 words in front of the workspace: [0], [1] the hub list's
constexpr int kSegGroups = 8192;  // lane groups of the segment kernels (stride over the slots)

// the caller's workspace, carved
struct Lists {
    int32_t *counters;    // kCounters words, zeroed by a memset on the stream in front of the first kernel
    float *part_val;      // [cap_seg, F] a segment's value (forward, in the flipped domain) or sum (backward)
    int32_t *part_pos;    // [cap_seg, F] a segment's position (forward)
    HubList hubs;
};

// bytes the carving takes from the first 256-byte boundary on; the query adds 256 for a workspace at any address
size_t carve(int32_t n_rows, int64_t nnz, int32_t F, void *ws, Lists *out)
{
    Lists w{};
    w.hubs.size(n_rows, nnz);
    Carver c(ws ? aligned_base(ws) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);   // 64 bytes: the partials stay 16-byte aligned (F % 4 == 0)
    w.part_val = c.take<float>((size_t)w.hubs.cap_seg * F, 4);
    w.part_pos = c.take<int32_t>((size_t)w.hubs.cap_seg * F, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hubs.take_slots(c);
    if (out) *out = w;
    return c.bytes();
}

__device__ __forceinline__ float flip(float t, uint32_t sign) { return __uint_as_float(__float_as_uint(t) ^ sign); }
__device__ __forceinline__ float4 flip(float4 t, uint32_t s) { return make_float4(flip(t.x, s), flip(t.y, s), flip(t.z, s), flip(t.w, s)); }

// ---- forward -------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    int32_t n_rows, F;
    const int32_t *rowptr, *colidx;
    const float *vals, *X;
    int64_t ldx;
    uint32_t sign;   // 0: max; 0x80000000: min, the maximum of the sign-flipped values
    float *Y;
    int64_t ldy;
    int32_t *arg;
    int64_t lda;
};

// what is stored for a lane's features: the value with its own sign again, +0 where the row has no entry
__device__ __forceinline__ float stored(float val, int32_t pos, uint32_t sign) { return pos < 0 ? 0.f : flip(val, sign); }
__device__ __forceinline__ float4 stored(float4 v, int4 p, uint32_t s)
{
    return make_float4(stored(v.x, p.x, s), stored(v.y, p.y, s), stored(v.z, p.z, s), stored(v.w, p.w, s));
}

// B entries k .. k + B - 1 of the group's current window (positions lo + k, ...): all loads, then the compares in ascending position
template <int G, int VEC, int B>
__device__ __forceinline__ void fwd_batch(typename Piece<VEC>::F &val, typename Piece<VEC>::I &pos, int k, int64_t lo, int32_t myc, int gbase,
                                          const float *xf, const FwdArgs &a)
{
    using V = typename Piece<VEC>::F;
    int32_t c[B];
    V x[B];
    float v[B];
#pragma unroll
    for (int u = 0; u < B; u++) c[u] = __shfl(myc, gbase + k + u, 64);
#pragma unroll
    for (int u = 0; u < B; u++) {
        x[u] = *reinterpret_cast<const V *>(xf + (int64_t)c[u] * a.ldx);
        v[u] = a.vals ? a.vals[lo + k + u] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < B; u++) meet(val, pos, flip(a.vals ? mul(x[u], v[u]) : x[u], a.sign), (int32_t)(lo + k + u));
}

// the entries b .. e - 1 in ascending position meet (val, pos); every lane of the group runs every shuffle
template <int G, int VEC>
__device__ __forceinline__ void fwd_span(typename Piece<VEC>::F &val, typename Piece<VEC>::I &pos, int64_t b, int64_t e, int li, int gbase,
                                         const float *xf, const FwdArgs &a)
{
    for (int64_t lo = b; lo < e; lo += G) {
        int64_t q = lo + li;
        q = q < e ? q : e - 1;
        const int32_t myc = a.colidx[q];
        const int n = e - lo < G ? (int)(e - lo) : G;
        int k = 0;
        for (; k + 4 <= n; k += 4) fwd_batch<G, VEC, 4>(val, pos, k, lo, myc, gbase, xf, a);
        for (; k < n; k++) fwd_batch<G, VEC, 1>(val, pos, k, lo, myc, gbase, xf, a);
    }
}

// grid.x: blocks of 256 / G rows; grid.y: tiles of G * VEC features.  A row longer than S goes to the hub list (tile 0 lists it).
template <int G, int VEC>
__global__ __launch_bounds__(256) void fwd_rows_kernel(FwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) - li;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    const bool active = f0 < a.F;               // VEC == 4: F % 4 == 0, so the whole piece is inside the row
    const int64_t fa = active ? f0 : 0;         // lanes past the row read feature 0 and never store
    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (row >= a.n_rows) return;                // uniform in the lane group; shuffles only ever meet lanes of the own group
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    V val;
    P pos;
    clear(val);
    none(pos);
    fwd_span<G, VEC>(val, pos, b, e, li, gbase, a.X + fa, a);
    if (!active) return;
    *reinterpret_cast<V *>(a.Y + row * a.ldy + f0) = stored(val, pos, a.sign);
    if (a.arg) *reinterpret_cast<P *>(a.arg + row * a.lda + f0) = pos;
}

// The lane groups of the segment kernels stride over the hub list's slots.  body(b, e, at, ...): the segment's entries b .. e - 1 and
// the slot's place in the partials.
template <int G, int VEC, class Body>
__device__ __forceinline__ void for_group_segments(const int32_t *__restrict__ rowptr, int32_t F, const Lists &w, Body body)
{
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) - li;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    const bool active = f0 < F;
    const int64_t fa = active ? f0 : 0;
    for_hub_segments(w.hubs, rowptr, (int64_t)blockIdx.x * GROUPS + threadIdx.x / G, (int64_t)gridDim.x * GROUPS,
                     [&](int32_t, int32_t, int64_t, int64_t b, int64_t n, int64_t slot) { body(b, b + n, slot * F + f0, li, gbase, fa, active); });
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void fwd_seg_kernel(FwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    for_group_segments<G, VEC>(a.rowptr, a.F, w, [&](int64_t b, int64_t e, int64_t at, int li, int gbase, int64_t fa, bool active) {
        V val;
        P pos;
        clear(val);
        none(pos);
        fwd_span<G, VEC>(val, pos, b, e, li, gbase, a.X + fa, a);
        if (active) {
            *reinterpret_cast<V *>(w.part_val + at) = val;
            *reinterpret_cast<P *>(w.part_pos + at) = pos;
        }
    });
}

// a thread per (hub, feature): the segments meet in ascending order, so of equal values the smaller position stays
__global__ __launch_bounds__(256) void fwd_combine_kernel(FwdArgs a, Lists w)
{
    const int64_t total = listed_hubs(w.hubs) * a.F;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t h = idx / a.F, f = idx - h * a.F;
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t at = (int64_t)w.hubs.hub_seg0[h] * a.F + f;
        float val = 0.f;
        int32_t pos = -1;
        for (int64_t s = 0; s < nseg; s++) meet(val, pos, w.part_val[at + s * a.F], w.part_pos[at + s * a.F]);
        a.Y[(int64_t)row * a.ldy + f] = stored(val, pos, a.sign);
        if (a.arg) a.arg[(int64_t)row * a.lda + f] = pos;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    int32_t n_rows, F;            // of the transposed pattern
    const int32_t *rowptr, *colidx, *map;
    const float *vals;
    const int32_t *arg;
    int64_t lda;
    const float *G;
    int64_t ldg;
    int beta;
    float *dX;
    int64_t ldx;
};

// acc + t where the entry won the feature, acc itself where it did not
__device__ __forceinline__ float route(float acc, float t, int32_t won, int32_t p) { return won == p ? acc + t : acc; }
__device__ __forceinline__ float4 route(float4 acc, float4 t, int4 won, int32_t p)
{
    return make_float4(route(acc.x, t.x, won.x, p), route(acc.y, t.y, won.y, p), route(acc.z, t.z, won.z, p), route(acc.w, t.w, won.w, p));
}

// B entries k .. k + B - 1 from the top of the group's current window (entries top - k, top - k - 1, ...): all loads, then the adds
template <int G, int VEC, int B>
__device__ __forceinline__ void bwd_batch(typename Piece<VEC>::F &acc, int k, int32_t myi, int32_t myp, int gbase, int64_t fa, const BwdArgs &a)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    int32_t i[B], p[B];
    V g[B];
    P won[B];
    float v[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
        i[u] = __shfl(myi, gbase + k + u, 64);
        p[u] = __shfl(myp, gbase + k + u, 64);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
        won[u] = *reinterpret_cast<const P *>(a.arg + (int64_t)i[u] * a.lda + fa);
        g[u] = *reinterpret_cast<const V *>(a.G + (int64_t)i[u] * a.ldg + fa);
        v[u] = a.vals ? a.vals[p[u]] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < B; u++) acc = route(acc, a.vals ? mul(g[u], v[u]) : g[u], won[u], p[u]);
}

// one accumulator per feature over the entries e - 1 down to b
template <int G, int VEC>
__device__ __forceinline__ void bwd_span(typename Piece<VEC>::F &acc, int64_t b, int64_t e, int li, int gbase, int64_t fa, const BwdArgs &a)
{
    for (int64_t hi = e; hi > b; hi -= G) {
        int64_t q = hi - 1 - li;
        q = q >= b ? q : b;
        const int32_t myi = a.colidx[q], myp = a.map[q];
        const int n = hi - b < G ? (int)(hi - b) : G;
        int k = 0;
        for (; k + 4 <= n; k += 4) bwd_batch<G, VEC, 4>(acc, k, myi, myp, gbase, fa, a);
        for (; k < n; k++) bwd_batch<G, VEC, 1>(acc, k, myi, myp, gbase, fa, a);
    }
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void bwd_rows_kernel(BwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) - li;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    const bool active = f0 < a.F;
    const int64_t fa = active ? f0 : 0;
    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (row >= a.n_rows) return;
    const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
    if (e - b > kSeg) {
        if (li == 0 && blockIdx.y == 0) append(w.hubs, (int32_t)row, e - b);
        return;
    }
    V acc;
    clear(acc);
    bwd_span<G, VEC>(acc, b, e, li, gbase, fa, a);
    if (!active) return;
    V *dst = reinterpret_cast<V *>(a.dX + row * a.ldx + f0);
    *dst = a.beta ? add(*dst, acc) : acc;
}

template <int G, int VEC>
__global__ __launch_bounds__(256) void bwd_seg_kernel(BwdArgs a, Lists w)
{
    using V = typename Piece<VEC>::F;
    for_group_segments<G, VEC>(a.rowptr, a.F, w, [&](int64_t b, int64_t e, int64_t at, int li, int gbase, int64_t fa, bool active) {
        V acc;
        clear(acc);
        bwd_span<G, VEC>(acc, b, e, li, gbase, fa, a);
        if (active) *reinterpret_cast<V *>(w.part_val + at) = acc;
    });
}

// a thread per (hub, feature): ((seg_0 + seg_1) + seg_2) + ...
__global__ __launch_bounds__(256) void bwd_combine_kernel(BwdArgs a, Lists w)
{
    const int64_t total = listed_hubs(w.hubs) * a.F;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t h = idx / a.F, f = idx - h * a.F;
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)a.rowptr[row + 1] - a.rowptr[row] + kSeg - 1) / kSeg;
        const int64_t at = (int64_t)w.hubs.hub_seg0[h] * a.F + f;
        float z = w.part_val[at];
        for (int64_t s = 1; s < nseg; s++) z = z + w.part_val[at + s * a.F];
        float *dst = a.dX + (int64_t)row * a.ldx + f;
        *dst = a.beta ? *dst + z : z;
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

}  // namespace

GNNX_API int gnnx_spmm_csr_reduce_workspace(int32_t n_rows, int64_t nnz, int32_t n_feat, size_t *bytes)
{
    GNNX_REQUIRE(bytes, GNNX_ERR_INVALID_ARG, "null pointer");
    int rc = check_sizes(n_rows, 0, n_feat, nnz);
    if (rc) return rc;
    *bytes = 256 + carve(n_rows, nnz, n_feat, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_spmm_csr_reduce_f32(int op, int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr,
                                      const int32_t *d_colidx, const float *d_vals, const float *d_X, int64_t ldx, float *d_Y, int64_t ldy,
                                      int32_t *d_arg, int64_t lda, void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows, n_cols, n_feat, nnz);
    if (rc) return rc;
    GNNX_REQUIRE(op == GNNX_REDUCE_MAX || op == GNNX_REDUCE_MIN, GNNX_ERR_INVALID_ARG, "op %d is neither GNNX_REDUCE_MAX nor GNNX_REDUCE_MIN", op);
    GNNX_REQUIRE(ldx >= n_feat && ldy >= n_feat && (!d_arg || lda >= n_feat), GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (n_rows == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr && d_Y && (nnz == 0 || (d_colidx && d_X)), GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    const size_t need = 256 + carve(n_rows, nnz, n_feat, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    const bool vec = n_feat % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(d_X) && aligned16(d_Y) && (!d_arg || (lda % 4 == 0 && aligned16(d_arg)));
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    hipStream_t st = as_stream(stream);
    const FwdArgs a{n_rows, n_feat, d_rowptr, d_colidx, d_vals, d_X, ldx, op == GNNX_REDUCE_MIN ? 0x80000000u : 0u, d_Y, ldy, d_arg, lda};
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    GNNX_DISPATCH_SHAPE(launch_fwd, sh, a, w, sh.tiles, st)
}

GNNX_API int gnnx_spmm_csr_reduce_bwd_f32(int32_t n_rows_t, int32_t n_cols_t, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr_t,
                                          const int32_t *d_colidx_t, const int32_t *d_map_t, const float *d_vals, const int32_t *d_arg,
                                          int64_t lda, const float *d_G, int64_t ldg, float beta, float *d_dX, int64_t ldx, void *d_workspace,
                                          size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(n_rows_t, n_cols_t, n_feat, nnz);
    if (rc) return rc;
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    GNNX_REQUIRE(lda >= n_feat && ldg >= n_feat && ldx >= n_feat, GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (n_rows_t == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(nnz == 0 || n_cols_t > 0, GNNX_ERR_INVALID_ARG, "entries in a matrix without columns");
    GNNX_REQUIRE(d_rowptr_t && d_dX && (nnz == 0 || (d_colidx_t && d_map_t && d_arg && d_G)), GNNX_ERR_INVALID_ARG, "null pointer");
    Lists w;
    const size_t need = 256 + carve(n_rows_t, nnz, n_feat, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    const bool vec = n_feat % 4 == 0 && lda % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && aligned16(d_arg) && aligned16(d_G) && aligned16(d_dX);
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    hipStream_t st = as_stream(stream);
    const BwdArgs a{n_rows_t, n_feat, d_rowptr_t, d_colidx_t, d_map_t, d_vals, d_arg, lda, d_G, ldg, beta != 0.f, d_dX, ldx};
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    GNNX_DISPATCH_SHAPE(launch_bwd, sh, a, w, sh.tiles, st)
}
