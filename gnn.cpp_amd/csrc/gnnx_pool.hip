// Graph readout: the SUM / MEAN / MAX of each segment of consecutive rows of X, and the backward that hands a segment's gradient back
// to its rows -- include/gnnx.h "graph readout".
//   forward:   segment b = rows [segptr[b], segptr[b+1]); chunks of T = GNNX_POOL_CHUNK rows counted from the segment's own first row;
//              a chunk is ONE accumulator per feature from +0 over its rows ascending (MAX: the first row, then strictly better rows),
//              the segment is ((c_0 + c_1) + c_2) + ... (MAX: the better chunk, on equal values the earlier one)
//   backward:  dX[i, f] = beta dX[i, f] + (G[b, f] | G[b, f] / len | arg[b, f] == i ? G[b, f] : +0)
// The work unit is a (segment, chunk) pair and there is no list of them: the grid is dealt over global TILES of T rows, tile t owning
// every chunk that STARTS in rows [t T, (t + 1) T).  A segment has at most one chunk start in a tile; of the segments longer than T at
// most two have one there -- the one that began before the tile (slot 2 t of the partials) and the one that begins inside it (slot
// 2 t + 1, and the tile notes that segment for the combine kernel).  Segments of at most T rows (the empty ones included: an empty
// segment "starts" at segptr[b] <= n_rows, which is why there are n_rows / T + 1 tiles) write Y directly.  How tiles map to lane
// groups is NOT in the result.  Lane shape of gnnx_reduce.hip: G = 4 .. 64 lanes per tile, lane l owns features f0 .. f0 + VEC - 1 of
// feature tile blockIdx.y; sixteen rows are requested before the first is added.  Every launch is on the caller's stream; nothing is
// allocated or synchronised, and no atomic exists in this file.
#include <type_traits>

#include "gnnx_lanes.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kT = GNNX_POOL_CHUNK;   // the contract's chunk length and the tile of the grid
constexpr int kAhead = 16;            // rows requested before the first of them is added
constexpr int kBwdRows = 32;          // consecutive rows of dX per lane group: one search in segptr serves them all
constexpr int kWide = 64;             // chunk partials the combine requests at once on a long run of chunks,
constexpr int kNarrow = 8;            // and behind it (or for a segment of few chunks)

// the caller's workspace, carved
struct Parts {
    float *val;          // [2 tiles, F] a chunk's sum or its maximum
    int32_t *pos;        // [2 tiles, F] the row of that maximum
    int32_t *long_seg;   // [tiles] the segment longer than T that starts in the tile; -1: none
    int64_t tiles;
};

// bytes the carving takes from the first 256-byte boundary on; the query adds 256 for a workspace at any address
size_t carve(int32_t n_rows, int32_t F, void *ws, Parts *out)
{
    Parts w{};
    w.tiles = (int64_t)n_rows / kT + 1;
    Carver c(ws ? aligned_base(ws) : nullptr);
    const size_t slab = 2 * (size_t)w.tiles * (size_t)F;   // words: a multiple of 16 bytes whenever F % 4 == 0
    w.val = c.take<float>(slab, 4);
    w.pos = c.take<int32_t>(slab, 4);
    w.long_seg = c.take<int32_t>((size_t)w.tiles, 4);
    if (out) *out = w;
    return c.bytes();
}

__device__ __forceinline__ float div(float a, float d) { return __fdiv_rn(a, d); }
__device__ __forceinline__ float4 div(float4 a, float d) { return make_float4(__fdiv_rn(a.x, d), __fdiv_rn(a.y, d), __fdiv_rn(a.z, d), __fdiv_rn(a.w, d)); }

// what MAX stores: +0 where the segment has no row
__device__ __forceinline__ float stored(float val, int32_t pos) { return pos < 0 ? 0.f : val; }
__device__ __forceinline__ float4 stored(float4 v, int4 p) { return make_float4(stored(v.x, p.x), stored(v.y, p.y), stored(v.z, p.z), stored(v.w, p.w)); }

// ---- forward -------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    int op;
    int32_t n_seg, n_rows, F;
    const int32_t *segptr;
    const float *X;
    int64_t ldx;
    float *Y;
    int64_t ldy;
    int32_t *arg;
    int64_t lda;
};

// rows r .. r + n - 1 (1 <= n <= B; FULL: n == B) in ascending order meet (val, pos): B rows are requested, then added (compared) one
// after the other.  A short batch requests its last row again in the slots behind it and passes those over: no second round trip.
template <int VEC, bool MAX, int B, bool FULL>
__device__ __forceinline__ void rows_batch(typename Piece<VEC>::F &val, typename Piece<VEC>::I &pos, int64_t r, int n, const float *xf, int64_t ldx)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    V x[B];
#pragma unroll
    for (int u = 0; u < B; u++) x[u] = *reinterpret_cast<const V *>(xf + (r + (FULL || u < n ? u : n - 1)) * ldx);
#pragma unroll
    for (int u = 0; u < B; u++) {
        V v = val;
        P p = pos;
        if constexpr (MAX) meet(v, p, x[u], (int32_t)(r + u));
        else v = add(v, x[u]);
        if (FULL || u < n) {
            val = v;
            pos = p;
        }
    }
}

template <int VEC, bool MAX>
__device__ __forceinline__ void chunk_rows(typename Piece<VEC>::F &val, typename Piece<VEC>::I &pos, int64_t b, int64_t e, const float *xf, int64_t ldx)
{
    clear(val);
    none(pos);
    int64_t r = b;
    for (; r + kAhead <= e; r += kAhead) rows_batch<VEC, MAX, kAhead, true>(val, pos, r, kAhead, xf, ldx);
    if (r < e) rows_batch<VEC, MAX, kAhead, false>(val, pos, r, (int)(e - r), xf, ldx);
}

// grid.x: blocks of 256 / G tiles; grid.y: tiles of G * VEC features
template <int G, int VEC, bool MAX>
__global__ __launch_bounds__(256) void fwd_tiles_kernel(FwdArgs a, Parts w)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    if (f0 >= a.F) return;                      // no lane of this kernel talks to another (VEC == 4: F % 4 == 0, the piece is whole)
    const int64_t tile = (int64_t)blockIdx.x * GROUPS + threadIdx.x / G;
    if (tile >= w.tiles) return;
    const int64_t lo = tile * kT, hi = lo + kT;   // lo <= n_rows: the last tile holds the empty segments at the very end
    const float *xf = a.X + f0;
    // the first segment that starts at or behind lo (segptr[n_seg] = n_rows >= lo: there is one among the n_seg + 1 entries)
    int32_t l = 0, r = a.n_seg;
    while (l < r) {
        const int32_t m = l + (r - l) / 2;
        if (a.segptr[m] < lo) l = m + 1; else r = m;
    }
    V val;
    P pos;
    // the segment that began before the tile: its chunk that starts here, if it has one, is never its first -- a partial
    if (l > 0) {
        const int64_t s = a.segptr[l - 1], e = a.segptr[l] < a.n_rows ? a.segptr[l] : a.n_rows;
        const int64_t b = s + (lo - s + kT - 1) / kT * kT;   // in [lo, hi)
        if (b < e) {
            chunk_rows<VEC, MAX>(val, pos, b, b + kT < e ? b + kT : e, xf, a.ldx);
            *reinterpret_cast<V *>(w.val + (2 * tile) * a.F + f0) = val;
            if constexpr (MAX) *reinterpret_cast<P *>(w.pos + (2 * tile) * a.F + f0) = pos;
        }
    }
    // the segments that start inside the tile, their first chunk
    int32_t long_seg = -1;
    int64_t s = l < a.n_seg ? a.segptr[l] : hi;
    for (int32_t b = l; b < a.n_seg && s < hi; b++) {
        const int64_t e_raw = a.segptr[b + 1];
        const int64_t e = e_raw < a.n_rows ? e_raw : a.n_rows;
        const bool whole = e - s <= kT;
        chunk_rows<VEC, MAX>(val, pos, s, whole ? e : s + kT, xf, a.ldx);
        if (!whole) long_seg = b;
        if (whole) {
            if constexpr (MAX) {
                *reinterpret_cast<V *>(a.Y + (int64_t)b * a.ldy + f0) = stored(val, pos);
                if (a.arg) *reinterpret_cast<P *>(a.arg + (int64_t)b * a.lda + f0) = pos;
            } else {
                *reinterpret_cast<V *>(a.Y + (int64_t)b * a.ldy + f0) = (a.op == GNNX_POOL_MEAN && e > s) ? div(val, (float)(e - s)) : val;
            }
        } else {
            *reinterpret_cast<V *>(w.val + (2 * tile + 1) * a.F + f0) = val;
            if constexpr (MAX) *reinterpret_cast<P *>(w.pos + (2 * tile + 1) * a.F + f0) = pos;
        }
        s = e_raw;
    }
    if (li == 0 && blockIdx.y == 0) w.long_seg[tile] = long_seg;
}

// a thread per (tile, feature): the long segment that starts in the tile, its chunks in ascending order.  Chunk 0 sits in the tile's
// second slot, chunk k >= 1 starts at row s + k T of tile s / T + k and sits in that tile's first slot.
template <bool MAX>
__global__ __launch_bounds__(256) void fwd_combine_kernel(FwdArgs a, Parts w)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= w.tiles * a.F) return;
    const int64_t tile = idx / a.F, f = idx - tile * a.F;
    const int32_t seg = w.long_seg[tile];
    if (seg < 0) return;
    const int64_t s = a.segptr[seg], e = a.segptr[seg + 1] < a.n_rows ? a.segptr[seg + 1] : a.n_rows;
    const int64_t n_chunks = (e - s + kT - 1) / kT;
    const int64_t F = a.F;
    float val = w.val[(2 * tile + 1) * F + f];
    int32_t pos = MAX ? w.pos[(2 * tile + 1) * F + f] : 0;
    const int64_t at = 2 * tile * F + f;   // chunk k: at + 2 k F
    // n chunks from k on (FULL: n == B): all requests first -- this thread is one of few, the round trips are its whole cost
    auto batch = [&](auto full, auto width, int64_t k, int n) {
        constexpr int B = decltype(width)::value;
        constexpr bool FULL = decltype(full)::value;
        float v[B];
        int32_t p[B];
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int64_t o = at + 2 * (k + (FULL || u < n ? u : n - 1)) * F;
            v[u] = w.val[o];
            if constexpr (MAX) p[u] = w.pos[o];
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            if (FULL || u < n) {
                if constexpr (MAX) meet(val, pos, v[u], p[u]);
                else val = val + v[u];
            }
        }
    };
    int64_t k = 1;
    for (; k + kWide <= n_chunks; k += kWide) batch(std::true_type{}, std::integral_constant<int, kWide>{}, k, kWide);
    for (; k < n_chunks; k += kNarrow)
        batch(std::false_type{}, std::integral_constant<int, kNarrow>{}, k, n_chunks - k < kNarrow ? (int)(n_chunks - k) : kNarrow);
    if constexpr (MAX) {
        a.Y[(int64_t)seg * a.ldy + f] = val;
        if (a.arg) a.arg[(int64_t)seg * a.lda + f] = pos;
    } else {
        a.Y[(int64_t)seg * a.ldy + f] = a.op == GNNX_POOL_MEAN ? __fdiv_rn(val, (float)(e - s)) : val;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    int32_t n_seg, n_rows, F;
    const int32_t *segptr, *arg;
    int64_t lda;
    const float *G;
    int64_t ldg;
    int beta;
    float *dX;
    int64_t ldx;
};

__device__ __forceinline__ float won(float g, int32_t a, int32_t i) { return a == i ? g : 0.f; }
__device__ __forceinline__ float4 won(float4 g, int4 a, int32_t i) { return make_float4(won(g.x, a.x, i), won(g.y, a.y, i), won(g.z, a.z, i), won(g.w, a.w, i)); }

// grid.x: blocks of 256 / G runs of kBwdRows rows; grid.y: tiles of G * VEC features
template <int G, int VEC, int OP>
__global__ __launch_bounds__(256) void bwd_rows_kernel(BwdArgs a)
{
    using V = typename Piece<VEC>::F;
    using P = typename Piece<VEC>::I;
    constexpr int GROUPS = 256 / G;
    const int li = threadIdx.x % G;
    const int64_t f0 = ((int64_t)blockIdx.y * G + li) * VEC;
    if (f0 >= a.F) return;                      // no lane of this kernel talks to another
    const int64_t row0 = ((int64_t)blockIdx.x * GROUPS + threadIdx.x / G) * kBwdRows;
    if (row0 >= a.n_rows) return;
    const int64_t row1 = row0 + kBwdRows < a.n_rows ? row0 + kBwdRows : a.n_rows;
    // the segment of row0: the last one that starts at or before it and is not empty (segptr[0] = 0 <= row0 < n_rows = segptr[n_seg])
    int32_t l = 0, r = a.n_seg;
    while (l < r) {
        const int32_t m = l + (r - l) / 2;
        if (a.segptr[m] <= row0) l = m + 1; else r = m;
    }
    int32_t b = l > 0 ? l - 1 : 0;
    int64_t e = a.segptr[b + 1];
    int32_t loaded = -1;
    V g;
    P arg;
    clear(g);
    none(arg);
    for (int64_t i = row0; i < row1; i++) {
        while (i >= e && b + 1 < a.n_seg) e = a.segptr[++b + 1];
        if (b != loaded) {
            g = *reinterpret_cast<const V *>(a.G + (int64_t)b * a.ldg + f0);
            if constexpr (OP == GNNX_POOL_MEAN) g = div(g, (float)(e - a.segptr[b]));
            if constexpr (OP == GNNX_POOL_MAX) arg = *reinterpret_cast<const P *>(a.arg + (int64_t)b * a.lda + f0);
            loaded = b;
        }
        V t = g;
        if constexpr (OP == GNNX_POOL_MAX) t = won(g, arg, (int32_t)i);
        V *dst = reinterpret_cast<V *>(a.dX + i * a.ldx + f0);
        *dst = a.beta ? add(*dst, t) : t;
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

template <int G, int VEC>
int launch_fwd(const FwdArgs &a, const Parts &w, uint32_t ftiles, hipStream_t st)
{
    const dim3 grid((uint32_t)ceil_div(w.tiles, 256 / G), ftiles);
    const uint32_t combine = (uint32_t)ceil_div(w.tiles * a.F, 256);
    if (a.op == GNNX_POOL_MAX) {
        hipLaunchKernelGGL((fwd_tiles_kernel<G, VEC, true>), grid, dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
        if (a.n_rows > kT) hipLaunchKernelGGL(fwd_combine_kernel<true>, dim3(combine), dim3(256), 0, st, a, w);
    } else {
        hipLaunchKernelGGL((fwd_tiles_kernel<G, VEC, false>), grid, dim3(256), 0, st, a, w);
        GNNX_LAUNCH_CHECK();
        if (a.n_rows > kT) hipLaunchKernelGGL(fwd_combine_kernel<false>, dim3(combine), dim3(256), 0, st, a, w);
    }
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

template <int G, int VEC>
int launch_bwd(int op, const BwdArgs &a, uint32_t ftiles, hipStream_t st)
{
    const dim3 grid((uint32_t)ceil_div(ceil_div(a.n_rows, kBwdRows), 256 / G), ftiles);
    if (op == GNNX_POOL_SUM) hipLaunchKernelGGL((bwd_rows_kernel<G, VEC, GNNX_POOL_SUM>), grid, dim3(256), 0, st, a);
    else if (op == GNNX_POOL_MEAN) hipLaunchKernelGGL((bwd_rows_kernel<G, VEC, GNNX_POOL_MEAN>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((bwd_rows_kernel<G, VEC, GNNX_POOL_MAX>), grid, dim3(256), 0, st, a);
    GNNX_LAUNCH_CHECK();
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
int check_sizes(int op, int32_t n_seg, int32_t n_rows, int32_t n_feat)
{
    GNNX_REQUIRE(n_seg >= 0 && n_rows >= 0 && n_feat >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(op == GNNX_POOL_SUM || op == GNNX_POOL_MEAN || op == GNNX_POOL_MAX, GNNX_ERR_INVALID_ARG,
                 "op %d is none of GNNX_POOL_SUM, GNNX_POOL_MEAN, GNNX_POOL_MAX", op);
    GNNX_REQUIRE(n_seg > 0 || n_rows == 0, GNNX_ERR_INVALID_ARG, "%d rows in no segment", n_rows);
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_segment_pool_workspace(int32_t n_seg, int32_t n_rows, int32_t n_feat, size_t *bytes)
{
    GNNX_REQUIRE(bytes, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(n_seg >= 0 && n_rows >= 0 && n_feat >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    *bytes = 256 + carve(n_rows, n_feat, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_segment_pool_f32(int op, int32_t n_seg, int32_t n_rows, int32_t n_feat, const int32_t *d_segptr, const float *d_X,
                                   int64_t ldx, float *d_Y, int64_t ldy, int32_t *d_arg, int64_t lda, void *d_workspace,
                                   size_t workspace_bytes, void *stream)
{
    int rc = check_sizes(op, n_seg, n_rows, n_feat);
    if (rc) return rc;
    GNNX_REQUIRE(ldx >= n_feat && ldy >= n_feat && (op != GNNX_POOL_MAX || !d_arg || lda >= n_feat), GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (n_seg == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_Y && (d_X || n_rows == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    Parts w;
    const size_t need = 256 + carve(n_rows, n_feat, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    int32_t *arg = op == GNNX_POOL_MAX ? d_arg : nullptr;   // SUM and MEAN never write it
    const bool vec = n_feat % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(d_X) && aligned16(d_Y) && (!arg || (lda % 4 == 0 && aligned16(arg)));
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536 && w.tiles * n_feat / 256 < (1ll << 31), GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    const FwdArgs a{op, n_seg, n_rows, n_feat, d_segptr, d_X, ldx, d_Y, ldy, arg, lda};
    GNNX_DISPATCH_SHAPE(launch_fwd, sh, a, w, sh.tiles, as_stream(stream))
}

GNNX_API int gnnx_segment_pool_bwd_f32(int op, int32_t n_seg, int32_t n_rows, int32_t n_feat, const int32_t *d_segptr, const int32_t *d_arg,
                                       int64_t lda, const float *d_G, int64_t ldg, float beta, float *d_dX, int64_t ldx, void *stream)
{
    int rc = check_sizes(op, n_seg, n_rows, n_feat);
    if (rc) return rc;
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    const bool max = op == GNNX_POOL_MAX;
    GNNX_REQUIRE(ldg >= n_feat && ldx >= n_feat && (!max || lda >= n_feat), GNNX_ERR_INVALID_ARG, "ld < n_feat");
    if (n_seg == 0 || n_feat == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_G && (!max || d_arg) && (d_dX || n_rows == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;   // no row of dX to write
    const bool vec = n_feat % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && aligned16(d_G) && aligned16(d_dX) && (!max || (lda % 4 == 0 && aligned16(d_arg)));
    const Shape sh = shape_of(n_feat, vec);
    GNNX_REQUIRE(sh.tiles < 65536, GNNX_ERR_UNSUPPORTED, "n_feat too wide for one launch");
    const BwdArgs a{n_seg, n_rows, n_feat, d_segptr, max ? d_arg : nullptr, lda, d_G, ldg, beta != 0.f, d_dX, ldx};
    GNNX_DISPATCH_SHAPE(launch_bwd, sh, op, a, sh.tiles, as_stream(stream))
}
