// k nearest neighbours by exact all-pairs distances -- include/gnnx.h "nearest neighbours".
//   * a workgroup is ONE wavefront that owns 64 / G consecutive queries, G lanes (a power of two) per query, and strides over the query
//     blocks.  Queries of one block that lie in different segments are served segment by segment (a pass per segment the block touches,
//     the other lanes idle): a candidate tile never crosses a segment.
//   * the distance: a tile of candidate rows is staged in LDS; lane r of a group takes the tile's rows r, r + G, ... -- at G = 1 every
//     lane reads the same address (a broadcast).  Register form (n_feat <= GNNX_KNN_REG_FEAT): the query row sits in NF registers, NF the
//     smallest of {2, 3, 4, 8, 16, 32, 64} that holds it, tiles of GNNX_KNN_TILE rows.  LDS form (beyond): tiles of GNNX_KNN_TILE_LDS
//     rows, 64 features of the tile and of the block's queries staged at a time, one accumulator per row of the lane's share.  Columns
//     behind n_feat are zero on both sides: (0 - 0)^2 = +0, and acc + (+0) is acc for every acc the chain can hold (never -0), so the
//     padding changes no bit.  Contraction is off in this unit whatever the command line says (the pragma below).
//   * the selection: every lane keeps its k smallest keys ASCENDING in a slice of LDS (entry j of lane l at word j * 64 + l: no bank
//     conflict) and the k-th in a register; a candidate is inserted only when its key is below that -- rare after the first tile.  Empty
//     places hold ~0, which is above every key.  The G lists of a query are then merged pairwise in log2 G rounds, IN PLACE: a forward
//     pass counts how many of the k smallest come from each list, a backward pass writes them from the top, so no entry is overwritten
//     before it is read.  Keys are distinct and totally ordered: the result cannot depend on G or on the split.
//   * the output: the group's first lane holds the result in ascending key order (NEAREST_FIRST as it is); ascending index order is a
//     rank count over the k entries.
// 64-bit offsets, no atomics, no workspace.  Plain C++ and vector stores only.
#include "gnnx_common.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kMaxK = GNNX_KNN_MAX_K;
constexpr int kTile = GNNX_KNN_TILE;
constexpr int kTileLds = GNNX_KNN_TILE_LDS;
constexpr int kRegFeat = GNNX_KNN_REG_FEAT;
constexpr int kChunkF = 64;                 // LDS form: features staged at a time
constexpr int kPitchX = kChunkF + 4;        // LDS form: tile row pitch (rows stay 16-byte aligned)
constexpr int kPitchQ = kChunkF + 1;        // LDS form: query row pitch (a column read by 64 slots hits 64 banks)
constexpr uint64_t kEmpty = ~0ull;          // above every key: ukey <= 0xFFFFFFFF and the index is below 2^31
static_assert(kTile == 64 && kTileLds == 16 && kRegFeat == 64 && kMaxK <= 64, "the layouts below");

struct Args {
    int32_t n, m, n_feat, n_seg, k;
    int32_t gs;                             // log2 of the lanes per query
    uint32_t flags;
    const float *X, *Q;
    int64_t ldx, ldq;
    const int32_t *segptr, *qsegptr;        // both null: one segment
    int32_t *idx;
    float *dist;
    int64_t ldi, ldd;
};

__device__ __forceinline__ uint64_t make_key(float d, int64_t c)
{
    const uint32_t u = d != d ? 0xFFFFFFFFu : __float_as_uint(d);
    return ((uint64_t)u << 32) | (uint64_t)(uint32_t)c;
}

// the stored distance of a key: its bits, a NaN as the canonical quiet NaN
__device__ __forceinline__ float dist_of(uint64_t key)
{
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float(u == 0xFFFFFFFFu ? 0x7FC00000u : u);
}

// the largest b in [0, n_seg) with ptr[b] <= i (ptr[0] == 0 <= i): the segment that holds i, empty segments skipped
__device__ __forceinline__ int32_t seg_of(const int32_t *ptr, int32_t n_seg, int64_t i)
{
    int32_t lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)ptr[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// key < kth (the lane's k-th smallest, mine[(k - 1) * 64]) takes its place in the ascending list
__device__ __forceinline__ void insert(uint64_t *mine, int k, uint64_t key, uint64_t &kth)
{
    int j = k - 1;
    while (j > 0) {
        const uint64_t below = mine[(j - 1) * 64];
        if (below <= key) break;
        mine[j * 64] = below;
        j--;
    }
    mine[j * 64] = key;
    kth = mine[(k - 1) * 64];
}

// a <- the k smallest of a and b (both ascending, k entries), ascending, in place
__device__ __forceinline__ void merge_into(uint64_t *a, const uint64_t *b, int k)
{
    int na = 0, nb = 0;
    for (int t = 0; t < k; t++) {      // na + nb == t < k: both reads are inside the lists
        if (a[na * 64] <= b[nb * 64]) na++;
        else nb++;
    }
    int ia = na - 1, ib = nb - 1, p = k - 1;   // p == ia + ib + 1 > ia while ib >= 0: a write never reaches an unread entry of a
    while (ib >= 0) {
        const uint64_t vb = b[ib * 64];
        if (ia >= 0) {
            const uint64_t va = a[ia * 64];
            if (va > vb) {
                a[p * 64] = va;
                p--, ia--;
                continue;
            }
        }
        a[p * 64] = vb;
        p--, ib--;
    }
}

// the merge rounds of a pass and the rows of its queries; `mine` of a group's first lane ends as the query's ascending list
__device__ __forceinline__ void finish(const Args &A, uint64_t *mine, bool active, int r, int64_t qi)
{
    const int k = A.k, G = 1 << A.gs;
    __syncthreads();
    for (int s = 1; s < G; s <<= 1) {
        if (active && (r & (2 * s - 1)) == 0) merge_into(mine, mine + s, k);
        __syncthreads();
    }
    if (active && r == 0) {
        int32_t *oi = A.idx + qi * A.ldi;
        float *od = A.dist ? A.dist + qi * A.ldd : nullptr;
        const bool by_key = (A.flags & GNNX_KNN_NEAREST_FIRST) != 0;
        for (int i = 0; i < k; i++) {
            const uint64_t key = mine[i * 64];
            int at = i;
            if (key != kEmpty && !by_key) {   // the number of kept indices below this one
                at = 0;
                for (int j = 0; j < k; j++) {
                    const uint64_t other = mine[j * 64];
                    if (other == kEmpty) break;
                    at += (uint32_t)other < (uint32_t)key;
                }
            }
            oi[at] = key == kEmpty ? -1 : (int32_t)(uint32_t)key;
            if (od) od[at] = key == kEmpty ? __uint_as_float(0x7F800000u) : dist_of(key);
        }
    }
    __syncthreads();
}

// what a block's pass over segment b covers: queries [ql, qh) of the block's [q0, q1), candidates [cl, ch)
struct Pass {
    int64_t ql, qh, cl, ch;
};

__device__ __forceinline__ Pass pass_of(const Args &A, int32_t b, int64_t q0, int64_t q1)
{
    Pass p{0, A.m, 0, A.n};
    if (A.qsegptr) {
        p.ql = A.qsegptr[b], p.qh = A.qsegptr[b + 1];
        p.cl = A.segptr[b], p.ch = A.segptr[b + 1];
    }
    p.ql = p.ql < q0 ? q0 : p.ql;
    p.qh = p.qh > q1 ? q1 : p.qh;
    p.cl = p.cl < 0 ? 0 : p.cl;                 // (the arrays are trusted; a bad one still reads no row outside X)
    p.ch = p.ch > A.n ? (int64_t)A.n : p.ch;
    return p;
}

template <int NF>
__global__ __launch_bounds__(64) void knn_reg_kernel(Args A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int P = NF >= 4 ? NF + 4 : NF;                       // tile row pitch: 16-byte rows that start on different banks
    constexpr int FL = NF <= 2 ? 2 : NF <= 4 ? 4 : NF;             // lanes that stage one row (a power of two)
    const int lane = threadIdx.x, k = A.k;
    const int G = 1 << A.gs, nq = 64 >> A.gs, slot = lane >> A.gs, r = lane & (G - 1);
    uint64_t *mine = reinterpret_cast<uint64_t *>(smem) + lane;
    float *xs = reinterpret_cast<float *>(smem + (size_t)k * 64 * sizeof(uint64_t));   // [kTile][P]
    const bool no_self = (A.flags & GNNX_KNN_EXCLUDE_SELF) != 0;
    for (int e = lane; e < kTile * P; e += 64) xs[e] = 0.f;        // the columns behind n_feat stay zero
    const int64_t n_blocks = ((int64_t)A.m + nq - 1) >> (6 - A.gs);
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t q0 = blk * nq, q1 = q0 + nq < A.m ? q0 + nq : (int64_t)A.m, qi = q0 + slot;
        const int32_t b0 = A.qsegptr ? seg_of(A.qsegptr, A.n_seg, q0) : 0, b1 = A.qsegptr ? seg_of(A.qsegptr, A.n_seg, q1 - 1) : 0;
        for (int32_t b = b0; b <= b1; b++) {
            const Pass ps = pass_of(A, b, q0, q1);
            if (ps.ql >= ps.qh) continue;      // (the same in every lane)
            const bool active = qi >= ps.ql && qi < ps.qh;
            float q[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) q[f] = active && f < A.n_feat ? A.Q[qi * A.ldq + f] : 0.f;
            for (int j = 0; j < k; j++) mine[j * 64] = kEmpty;
            uint64_t kth = kEmpty;
            for (int64_t c0 = ps.cl; c0 < ps.ch; c0 += kTile) {
                const int cnt = ps.ch - c0 < kTile ? (int)(ps.ch - c0) : kTile;
                __syncthreads();   // the tile's readers are through
                {
                    const int f = lane & (FL - 1);
                    if (f < A.n_feat)
                        for (int c = lane / FL; c < cnt; c += 64 / FL) xs[c * P + f] = A.X[(c0 + c) * A.ldx + f];
                }
                __syncthreads();
                if (active) {
                    for (int c = r; c < cnt; c += G) {
                        const int64_t cg = c0 + c;
                        if (no_self && cg == qi) continue;
                        const float *x = xs + c * P;
                        float acc = 0.f;
#pragma unroll
                        for (int f = 0; f < NF; f++) {
                            const float t = q[f] - x[f];
                            const float p = t * t;
                            acc = acc + p;
                        }
                        const uint64_t key = make_key(acc, cg);
                        if (key < kth) insert(mine, k, key, kth);
                    }
                }
            }
            finish(A, mine, active, r, qi);
        }
    }
}

__global__ __launch_bounds__(64) void knn_lds_kernel(Args A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x, k = A.k;
    const int G = 1 << A.gs, nq = 64 >> A.gs, slot = lane >> A.gs, r = lane & (G - 1);
    const int share = kTileLds >> A.gs;        // rows of a tile per lane (G <= kTileLds)
    uint64_t *mine = reinterpret_cast<uint64_t *>(smem) + lane;
    float *xs = reinterpret_cast<float *>(smem + (size_t)k * 64 * sizeof(uint64_t));   // [kTileLds][kPitchX]
    float *qs = xs + kTileLds * kPitchX;                                                // [64][kPitchQ], row = query slot
    const bool no_self = (A.flags & GNNX_KNN_EXCLUDE_SELF) != 0;
    const int64_t n_blocks = ((int64_t)A.m + nq - 1) >> (6 - A.gs);
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t q0 = blk * nq, q1 = q0 + nq < A.m ? q0 + nq : (int64_t)A.m, qi = q0 + slot;
        const int32_t b0 = A.qsegptr ? seg_of(A.qsegptr, A.n_seg, q0) : 0, b1 = A.qsegptr ? seg_of(A.qsegptr, A.n_seg, q1 - 1) : 0;
        for (int32_t b = b0; b <= b1; b++) {
            const Pass ps = pass_of(A, b, q0, q1);
            if (ps.ql >= ps.qh) continue;      // (the same in every lane)
            const bool active = qi >= ps.ql && qi < ps.qh;
            for (int j = 0; j < k; j++) mine[j * 64] = kEmpty;
            uint64_t kth = kEmpty;
            for (int64_t c0 = ps.cl; c0 < ps.ch; c0 += kTileLds) {
                const int cnt = ps.ch - c0 < kTileLds ? (int)(ps.ch - c0) : kTileLds;
                float acc[kTileLds];
#pragma unroll
                for (int i = 0; i < kTileLds; i++) acc[i] = 0.f;
                for (int32_t f0 = 0; f0 < A.n_feat; f0 += kChunkF) {
                    const int fc = A.n_feat - f0 < kChunkF ? A.n_feat - f0 : kChunkF;
                    __syncthreads();   // the chunk's readers are through
                    for (int c = 0; c < cnt; c++) xs[c * kPitchX + lane] = lane < fc ? A.X[(c0 + c) * A.ldx + f0 + lane] : 0.f;
                    for (int s = 0; s < nq; s++) {
                        const int64_t row = q0 + s;
                        qs[s * kPitchQ + lane] = lane < fc && row >= ps.ql && row < ps.qh ? A.Q[row * A.ldq + f0 + lane] : 0.f;
                    }
                    __syncthreads();
                    if (active) {
                        for (int f = 0; f < fc; f++) {
                            const float qv = qs[slot * kPitchQ + f];
#pragma unroll
                            for (int i = 0; i < kTileLds; i++) {
                                if (i < share) {   // (the same in every lane); rows behind cnt hold stale numbers that nobody keeps
                                    const float t = qv - xs[(r + (i << A.gs)) * kPitchX + f];
                                    const float p = t * t;
                                    acc[i] = acc[i] + p;
                                }
                            }
                        }
                    }
                }
                if (active) {
#pragma unroll
                    for (int i = 0; i < kTileLds; i++) {
                        const int c = r + (i << A.gs);
                        if (i < share && c < cnt) {
                            const int64_t cg = c0 + c;
                            const uint64_t key = make_key(acc[i], cg);
                            if (!(no_self && cg == qi) && key < kth) insert(mine, k, key, kth);
                        }
                    }
                }
            }
            finish(A, mine, active, r, qi);
        }
    }
}

size_t lds_reg(int k, int NF) { return (size_t)k * 64 * sizeof(uint64_t) + sizeof(float) * kTile * (NF >= 4 ? NF + 4 : NF); }
size_t lds_lds(int k) { return (size_t)k * 64 * sizeof(uint64_t) + sizeof(float) * (kTileLds * kPitchX + 64 * kPitchQ); }

template <int NF>
int launch_reg(const Args &a, dim3 grid, hipStream_t st)
{
    static std::atomic<uint64_t> done{0};
    const int rc = lds_opt_in(&knn_reg_kernel<NF>, lds_reg(kMaxK, NF), done, "knn_reg_kernel");   // the largest request of any k
    if (rc != GNNX_OK) return rc;
    hipLaunchKernelGGL((knn_reg_kernel<NF>), grid, dim3(64), lds_reg(a.k, NF), st, a);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

int launch_lds(const Args &a, dim3 grid, hipStream_t st)
{
    static std::atomic<uint64_t> done{0};
    const int rc = lds_opt_in(&knn_lds_kernel, lds_lds(kMaxK), done, "knn_lds_kernel");
    if (rc != GNNX_OK) return rc;
    hipLaunchKernelGGL(knn_lds_kernel, grid, dim3(64), lds_lds(a.k), st, a);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_knn_f32(int32_t n, int32_t m, int32_t n_feat, int32_t n_seg, const float *d_X, int64_t ldx, const int32_t *d_segptr,
                          const float *d_Q, int64_t ldq, const int32_t *d_qsegptr, int32_t k, uint32_t flags, int32_t *d_idx, int64_t ldi,
                          float *d_dist, int64_t ldd, void *stream)
{
    GNNX_REQUIRE(n >= 0 && m >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_feat >= 1, GNNX_ERR_INVALID_ARG, "n_feat %d < 1", n_feat);
    GNNX_REQUIRE(k >= 1 && k <= kMaxK, GNNX_ERR_INVALID_ARG, "k = %d outside 1 .. %d", k, kMaxK);
    GNNX_REQUIRE(n_seg >= 1, GNNX_ERR_INVALID_ARG, "n_seg %d < 1", n_seg);
    GNNX_REQUIRE((flags & ~(GNNX_KNN_EXCLUDE_SELF | GNNX_KNN_NEAREST_FIRST)) == 0, GNNX_ERR_INVALID_ARG, "unknown flag bits 0x%x", flags);
    GNNX_REQUIRE(ldx >= n_feat && (!d_Q || ldq >= n_feat), GNNX_ERR_INVALID_ARG, "ldx %lld or ldq %lld < n_feat %d", (long long)ldx,
                 (long long)ldq, n_feat);
    GNNX_REQUIRE(ldi >= k && (!d_dist || ldd >= k), GNNX_ERR_INVALID_ARG, "ldi %lld or ldd %lld < k %d", (long long)ldi, (long long)ldd, k);
    if (d_Q) {
        GNNX_REQUIRE(!d_segptr == !d_qsegptr, GNNX_ERR_INVALID_ARG, "one of the two segment arrays is null");
    } else {
        GNNX_REQUIRE(m == n, GNNX_ERR_INVALID_ARG, "the queries are the candidates (null d_Q) but m = %d, n = %d", m, n);
        d_Q = d_X, ldq = ldx, d_qsegptr = d_segptr;
    }
    GNNX_REQUIRE(d_segptr || n_seg == 1, GNNX_ERR_INVALID_ARG, "null segment arrays with n_seg = %d", n_seg);
    GNNX_REQUIRE((d_X || n == 0) && (d_idx || m == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    if (m == 0) return GNNX_OK;
    // the dispatch of include/gnnx.h: a function of the arguments alone
    int gs = 0;
    while (gs < 6 && ((int64_t)m << gs) < GNNX_KNN_FULL_LANES) gs++;
    int cap = 0;
    while (cap < 6 && ((int64_t)4 * k << cap) <= (int64_t)(n / n_seg)) cap++;   // G * 2k <= the mean segment: 2G <= mean / k
    gs = gs < cap ? gs : cap;
    // only G = 1 reads a tile row as a broadcast: G lanes on G rows cost G LDS reads, and wide rows are bound by them (measured)
    const int nf = n_feat > kRegFeat ? kChunkF : n_feat <= 4 ? (n_feat < 2 ? 2 : n_feat) : n_feat <= 8 ? 8 : n_feat <= 16 ? 16 : n_feat <= 32 ? 32 : 64;
    while (gs > 0 && (nf << gs) > GNNX_KNN_GROUP_FLOATS) gs--;
#ifdef GNNX_EXPERIMENTS
    if (const char *e = experiment_env("GNNX_KNN_GROUP_LOG2")) {   // scripts/bench_knn.py: what the lane groups buy
        gs = std::atoi(e);
        gs = gs < 0 ? 0 : gs > (n_feat > kRegFeat ? 4 : 6) ? (n_feat > kRegFeat ? 4 : 6) : gs;
    }
#endif
    const Args a{n, m, n_feat, n_seg, k, gs, flags, d_X, d_Q, ldx, ldq, d_segptr, d_qsegptr, d_idx, d_dist, ldi, ldd};
    const int64_t n_blocks = ceil_div(m, 64 >> gs);
    const dim3 grid((uint32_t)(n_blocks < (int64_t)kNumCU * 32 ? n_blocks : (int64_t)kNumCU * 32));
    hipStream_t st = as_stream(stream);
    if (n_feat > kRegFeat) return launch_lds(a, grid, st);
    if (n_feat <= 2) return launch_reg<2>(a, grid, st);
    if (n_feat == 3) return launch_reg<3>(a, grid, st);
    if (n_feat == 4) return launch_reg<4>(a, grid, st);
    if (n_feat <= 8) return launch_reg<8>(a, grid, st);
    if (n_feat <= 16) return launch_reg<16>(a, grid, st);
    if (n_feat <= 32) return launch_reg<32>(a, grid, st);
    return launch_reg<64>(a, grid, st);
}
