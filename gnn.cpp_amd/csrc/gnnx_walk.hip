// Random walks on a CSR -- include/gnnx.h "random walks".
//   * one lane per walk: a walk is a chain of dependent loads (rowptr[v], rowptr[v + 1], one colidx entry) and nothing of it can be
//     shared between lanes, so the only parallelism is the number of walks in flight.  A workgroup is ONE wavefront that owns 64
//     consecutive walks and strides over the walk blocks; a CU holds up to 32 of them, and the loads of the others hide a step's latency.
//   * the step: the 64-bit key of (seed, global walk number, step, attempt) is formed in registers; the uniform step is one
//     multiply-high and one load.  The node2vec step (Grover & Leskovec 2016) is KnightKing's rejection sampling (Yang et al. 2019): a
//     uniform candidate of the row is accepted against the integer threshold of its class -- the previous vertex, a neighbour of the
//     previous vertex (one binary search in that vertex's ascending row, skipped when both classes weigh the same), any other --, at
//     most GNNX_WALK_TRIES times; a step that accepts nothing takes the exact scan of the row's thresholds (two passes, one search per
//     entry).  The scan is the one piece the lanes share: once every lane is through its attempts the wavefront takes the pending
//     scans one walk at a time, 64 entries of the row per pass -- a hub row scanned by its own lane alone would hold the other 63 for
//     the whole of it.  Bounded: no attempt loop is longer than GNNX_WALK_TRIES, no scan longer than the row; there is no spin.
//   * the store: the wavefront keeps GNNX_WALK_CHUNK positions of its 64 walks in LDS (a lane writes its own row, pitch CHUNK + 1: no
//     bank conflict) and then stores the tile row piece by row piece, CHUNK adjacent lanes on the CHUNK contiguous words of one walk --
//     64-byte pieces at CHUNK = 16 where a lane storing its own row writes 4 bytes at a stride of ldw per step.  The pieces start at
//     any word (ldw and the chunk's first position are arbitrary), so the stores are one word per lane.
// Integer work, 64-bit offsets, no atomics, no workspace.  Plain C++ and vector stores only.
#include <cmath>

#include "gnnx_common.h"
#include "gnnx_rng.h"

using namespace gnnx;

namespace {

constexpr int kChunk = GNNX_WALK_CHUNK;
constexpr int kTries = GNNX_WALK_TRIES;
constexpr int kPitch = kChunk + 1;
constexpr uint64_t kDomain = 0x77616C6B73746570ull;   // "walkstep": independent of the neighbour and negative samplers under one seed
static_assert(kChunk >= 1 && kChunk <= 64 && (kChunk & (kChunk - 1)) == 0, "a row piece is dealt to a power-of-two group of lanes");

struct Args {
    int32_t n_rows, walk_length;
    int64_t n_walks, walk_base, ldw;
    uint64_t s;                       // splitmix64(seed ^ kDomain)
    uint64_t thr_a, thr_b, thr_c;     // candidate == previous vertex / stored in its row / otherwise; each <= 2^32
    const int32_t *rowptr, *colidx, *starts;
    int32_t *walks;
};

// h(w, t, a) of the contract from k = splitmix64(s ^ ((w << 32 | t) * golden))
__device__ __forceinline__ uint64_t draw(uint64_t k, uint32_t a) { return splitmix64(k ^ ((uint64_t)a * kGolden)); }

// the threshold of candidate x at a step that came from u, whose ascending row is c[0 .. ud)
__device__ __forceinline__ uint64_t threshold_of(const Args &A, int32_t x, int32_t u, const int32_t *c, int32_t ud)
{
    if (x == u) return A.thr_a;
    if (A.thr_b == A.thr_c) return A.thr_b;   // q == 1: the result cannot depend on the membership
    int32_t lo = 0, hi = ud;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (c[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return (lo < ud && c[lo] == x) ? A.thr_b : A.thr_c;
}

// the attempts of the node2vec step from v (row c_v[0 .. d), d >= 1) that came from u (row c_u[0 .. ud)): true and the step, or false
__device__ __forceinline__ bool rejection_step(const Args &A, uint64_t k, const int32_t *c_v, int32_t d, int32_t u, const int32_t *c_u, int32_t ud,
                                               int32_t &next)
{
    for (int a = 0; a < kTries; a++) {
        const int32_t x = c_v[__umul64hi(draw(k, 2 * a), (uint64_t)d)];
        if ((draw(k, 2 * a + 1) >> 32) < threshold_of(A, x, u, c_u, ud)) {
            next = x;
            return true;
        }
    }
    return false;
}

// the exact fallback of ONE walk's step, run by the whole wavefront with the same arguments in every lane: the row's thresholds are
// summed 64 entries at a time (integers: the sum has no order), then the first entry whose prefix sum exceeds r is found block by block
// with a lane scan.  Every lane returns the step.
__device__ __forceinline__ int32_t scan_step(const Args &A, int lane, uint64_t k, const int32_t *c_v, int32_t d, int32_t u, const int32_t *c_u,
                                             int32_t ud)
{
    unsigned long long W = 0;
    for (int64_t j = lane; j < d; j += 64) W += threshold_of(A, c_v[j], u, c_u, ud);
    for (int off = 32; off > 0; off >>= 1) W += __shfl_xor(W, off, 64);
    const uint64_t h = draw(k, 2 * kTries);
    if (W == 0) return c_v[__umul64hi(h, (uint64_t)d)];
    const uint64_t r = __umul64hi(h, W);   // < W: the scan below ends inside the row
    unsigned long long base = 0;
    for (int64_t j0 = 0; j0 < d; j0 += 64) {
        const int64_t j = j0 + lane;
        unsigned long long incl = j < d ? threshold_of(A, c_v[j], u, c_u, ud) : 0;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long below = __shfl_up(incl, off, 64);
            if (lane >= off) incl += below;
        }
        const unsigned long long hit = __ballot(j < d && base + incl > r);
        if (hit) return c_v[j0 + __ffsll((long long)hit) - 1];
        base += __shfl(incl, 63, 64);
    }
    return c_v[d - 1];   // (not reached)
}

// kUniform: p == 1 && q == 1 -- no loop and no search.  kStaged: the LDS tile; false is the naive store of the EXPERIMENTS build.
template <bool kUniform, bool kStaged>
__global__ __launch_bounds__(64) void walk_kernel(Args A)
{
    __shared__ int32_t tile[kStaged ? 64 * kPitch : 1];
    const int lane = threadIdx.x;
    const int64_t n_blocks = (A.n_walks + 63) >> 6;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t x0 = blk << 6;
        const int64_t x = x0 + lane;
        const bool mine = x < A.n_walks;
        const uint64_t w = (uint64_t)(A.walk_base + x);
        int32_t cur = -1, prev = -1;
        int64_t pb = 0;   // row `prev` is colidx[pb .. pb + pd)
        int32_t pd = 0;
        if (mine) {
            cur = A.starts[x];
            if ((uint32_t)cur >= (uint32_t)A.n_rows) cur = -1;
        }
        // position `pos` of every walk of the block, GNNX_WALK_CHUNK positions at a time; every lane runs every position (an ended
        // or surplus lane carries -1), so the barriers below are met by the whole wavefront
        for (int64_t pos0 = 0; pos0 <= A.walk_length; pos0 += kChunk) {
            const int32_t cnt = (int64_t)A.walk_length + 1 - pos0 < kChunk ? (int32_t)((int64_t)A.walk_length + 1 - pos0) : kChunk;
            for (int32_t c = 0; c < cnt; c++) {
                const int64_t pos = pos0 + c;
                if (pos > 0) {   // step t = pos - 1 from cur
                    int32_t next = -1, d = 0;
                    int64_t b = 0;
                    uint64_t k = 0;
                    bool scan = false;   // the attempts accepted nothing
                    if ((uint32_t)cur < (uint32_t)A.n_rows) {
                        b = A.rowptr[cur];
                        d = (int32_t)((int64_t)A.rowptr[cur + 1] - b);
                        if (d > 0) {
                            const uint32_t t = (uint32_t)(pos - 1);
                            k = splitmix64(A.s ^ (((w << 32) | t) * kGolden));
                            if (kUniform || t == 0) next = A.colidx[b + (int64_t)__umul64hi(draw(k, 0), (uint64_t)d)];
                            else scan = !rejection_step(A, k, A.colidx + b, d, prev, A.colidx + pb, pd, next);
                        }
                    }
                    if (!kUniform) {   // the wavefront is whole again here: it takes the pending fallbacks one walk at a time
                        for (unsigned long long pending = __ballot(scan); pending; pending &= pending - 1) {
                            const int src = __ffsll((long long)pending) - 1;
                            const int32_t got = scan_step(A, lane, __shfl((unsigned long long)k, src, 64), A.colidx + __shfl((long long)b, src, 64),
                                                          __shfl(d, src, 64), __shfl(prev, src, 64), A.colidx + __shfl((long long)pb, src, 64),
                                                          __shfl(pd, src, 64));
                            if (lane == src) next = got;
                        }
                    }
                    if (d > 0) prev = cur, pb = b, pd = d;
                    cur = next;
                }
                if (kStaged) tile[lane * kPitch + c] = cur;
                else if (mine) A.walks[x * A.ldw + pos] = cur;
            }
            if (kStaged) {
                __syncthreads();   // (one wavefront: the tile's writes are visible to its other lanes)
                const int col = lane & (kChunk - 1);
                for (int row = lane / kChunk; row < 64; row += 64 / kChunk)
                    if (col < cnt && x0 + row < A.n_walks) A.walks[(x0 + row) * A.ldw + pos0 + col] = tile[row * kPitch + col];
                __syncthreads();   // the tile is free for the next chunk
            }
        }
    }
}

// min(2^32, floor(weight / largest * 2^32)) -- the doubles of the contract
uint64_t threshold(double weight, double largest)
{
    const double v = std::floor(weight / largest * 4294967296.0);
    return v >= 4294967296.0 ? (1ull << 32) : (uint64_t)v;
}

}  // namespace

GNNX_API int gnnx_csr_random_walk(int32_t n_rows, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_starts,
                                  int64_t n_walks, int64_t walk_base, int32_t walk_length, double p, double q, uint64_t seed,
                                  int32_t *d_walks, int64_t ldw, void *stream)
{
    GNNX_REQUIRE(n_rows >= 0 && nnz >= 0 && n_walks >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(walk_length >= 0, GNNX_ERR_INVALID_ARG, "negative walk length %d", walk_length);
    GNNX_REQUIRE(ldw >= (int64_t)walk_length + 1, GNNX_ERR_INVALID_ARG, "ldw %lld < walk_length + 1 = %lld", (long long)ldw,
                 (long long)walk_length + 1);
    GNNX_REQUIRE(walk_base >= 0 && walk_base <= (1ll << 32) && n_walks <= (1ll << 32) - walk_base, GNNX_ERR_INVALID_ARG,
                 "walk numbers %lld .. +%lld do not fit 32 bits", (long long)walk_base, (long long)n_walks);
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(std::isfinite(p) && std::isfinite(q) && p > 0 && q > 0 && std::isfinite(1.0 / p) && std::isfinite(1.0 / q),
                 GNNX_ERR_INVALID_ARG, "p = %g and q = %g must be finite and positive (and so their reciprocals)", p, q);
    GNNX_REQUIRE(d_rowptr && ((d_starts && d_walks) || n_walks == 0) && (d_colidx || nnz == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_walks == 0) return GNNX_OK;
    const double wa = 1.0 / p, wb = 1.0, wc = 1.0 / q;
    const double M = std::fmax(wa, std::fmax(wb, wc));
    const Args a{n_rows,   walk_length, n_walks, walk_base, ldw, splitmix64(seed ^ kDomain), threshold(wa, M), threshold(wb, M), threshold(wc, M),
                 d_rowptr, d_colidx,    d_starts, d_walks};
    const int64_t n_blocks = ceil_div(n_walks, 64);
    const dim3 grid((uint32_t)(n_blocks < (int64_t)kNumCU * 32 ? n_blocks : (int64_t)kNumCU * 32));
    hipStream_t st = as_stream(stream);
    const bool uniform = p == 1.0 && q == 1.0;
#ifdef GNNX_EXPERIMENTS
    if (experiment_env("GNNX_WALK_DIRECT")) {   // scripts/bench_walks.py: what the LDS tile buys
        if (uniform) hipLaunchKernelGGL((walk_kernel<true, false>), grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((walk_kernel<false, false>), grid, dim3(64), 0, st, a);
        GNNX_LAUNCH_CHECK();
        return GNNX_OK;
    }
#endif
    if (uniform) hipLaunchKernelGGL((walk_kernel<true, true>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((walk_kernel<false, true>), grid, dim3(64), 0, st, a);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}
