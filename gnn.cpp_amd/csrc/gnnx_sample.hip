// Neighbour sampling: a fixed fanout of k entries per CSR row, uniformly without replacement, from a seed -- include/gnnx.h "neighbour
// sampling".  Entry j of row i carries the key
//   u_j = (h_j >> 32) << 32 | j,   h_j = splitmix64( splitmix64(seed) ^ ((i << 32 | j) * golden) )
// (the finaliser of gnnx_synth.hip); a row of d > k entries keeps the k entries with the smallest u_j, in stored order.  The u_j of a
// row are pairwise different, so "the k smallest" is a set with no tie rule and the result is a function of (seed, i, d, k) alone.
//   * lengths and scan: rowptr_out is the exclusive scan of min(d, k), made here by three small kernels over tiles of 1024 rows (tile
//     sums, a one-block scan of the sums, the rows of each tile) and not by rocprim: the scratch of a library scan is only known with
//     a device at hand, and this workspace is a closed formula of (n_rows, nnz, k) that the query evaluates on any host.  The total
//     goes to the host before anything is written to an output (a capacity that is too small writes nothing).
//   * rows of d <= L = 256: a lane group of G = 4 .. 64 lanes per row (G from the mean row length, as the feature count picks it in
//     gnnx_reduce.hip; 64 / G rows share a wavefront).  d <= k is a straight copy.  Otherwise the group finds the k-th smallest u by
//     a radix select on the 64-bit key from its top bit down: a pass counts the candidates (the entries that agree with the bits
//     fixed so far) whose next bit is 0 and descends into the half that holds the k-th; it stops as soon as as many candidates are
//     left as are still needed -- after about log2(d / k) + 2 passes, not 64.  Keys are recomputed in every pass and never stored.
//     The kept entries (u <= the threshold) are written in ascending j by a ballot-prefix compaction.
//   * long rows, L < d <= S = 4096: the row kernel appends them to a second list and a fixed grid gives each a wavefront of its own.
//     On a power-law graph they are few, sit next to each other (low ids) and cost hundreds of passes over a narrow lane group:
//     left in the row kernel they were 1.9 of the 2.0 ms of a call on the R-MAT graph of 10^6 vertices.
//   * hub rows, d > S: the row kernel appends them to the hub list (gnnx_worklist.h); a fixed grid of wavefronts strides over the
//     segments of S consecutive entries and writes the offsets j of each segment's min(k, len) smallest keys, ascending, to the
//     segment's slot; one wavefront per hub then selects the k smallest of the hub's candidates (every segment but the last gives
//     exactly k, so they are one contiguous ascending run) and writes the row.  The k smallest of a row are among the k smallest of
//     their segments.
//   * a row list (gnnx_csr_sample_rows): the same kernels with a row indirection.  Output row x samples CSR row rows[x]; the key is
//     formed from the CSR row, every offset, rowid and list entry from x.  The lists of long rows are sized for rows met once each:
//     a listed row that repeats more often than they hold is selected by the row kernel's own lane group.
// Integer work only.  Every loop is bounded by a row, segment or candidate length or by the 64 key bits; there is no spin wait.
#include "gnnx_rng.h"
#include "gnnx_worklist.h"

using namespace gnnx;

namespace {

constexpr int kLong = 256;         // L: rows longer than this (and not longer than S) get a wavefront of their own
constexpr int kMaxFanout = 64;     // one wavefront holds a segment's candidates
constexpr int kCounters = 16;      // int32 words in front of the workspace: [0], [1] the hub list's, [2] kept entries in all, [3] long rows,
                                   // [4] the range flag of a row list
constexpr int kSegWaves = 8192;    // wavefronts of the long-row, segment and combine kernels (stride over their lists)
constexpr int kScanTile = 1024;    // rows per block of the scan kernels: 4 per thread

// u_j of the contract; s = splitmix64(seed)
__device__ __forceinline__ uint64_t key_of(uint64_t s, uint32_t row, uint32_t j)
{
    const uint64_t h = splitmix64(s ^ ((((uint64_t)row << 32) | j) * kGolden));
    return (h & 0xFFFFFFFF00000000ull) | j;
}

// the caller's workspace, carved
struct Lists {
    int32_t *counters;    // kCounters words, zeroed by a memset on the stream in front of the first kernel
    int32_t *tile_sum;    // [n_tiles] kept entries of a tile of kScanTile rows, then their exclusive scan
    HubList hubs;
    int32_t *cand;        // [cap_seg, k] the offsets j of a segment's smallest keys, ascending
    int32_t *long_rows;   // [cap_long] rows of more than L and at most S entries
    int64_t n_tiles, cap_long;
};

// bytes the carving takes from the first 256-byte boundary on; the query adds 256 for a workspace at any address
size_t carve(int32_t n_rows, int64_t nnz, int32_t k, void *ws, Lists *out)
{
    Lists w{};
    w.n_tiles = (int64_t)n_rows / kScanTile + 1;   // tiles that cover the n_rows + 1 values of rowptr_out
    w.hubs.size(n_rows, nnz);
    w.cap_long = cap_rows_longer(n_rows, nnz, kLong);
    Carver c(ws ? aligned_base(ws) : nullptr);
    w.counters = c.take<int32_t>(kCounters, 4);
    w.tile_sum = c.take<int32_t>((size_t)w.n_tiles, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hubs.take_slots(c);
    w.cand = c.take<int32_t>((size_t)w.hubs.cap_seg * k, 4);
    w.long_rows = c.take<int32_t>((size_t)w.cap_long, 4);
    if (out) *out = w;
    return c.bytes();
}

// A call works on n_rows OUTPUT rows x.  Output row x samples row row_of(x) of the CSR: x itself for the whole graph, rows[x] with a
// row list (gnnx_csr_sample_rows).  The key is formed from the CSR row; offsets in the outputs, rowid and every list in the
// workspace are formed from x, so a row that the list repeats is two units of work with two outputs.
struct Args {
    int32_t n_rows, k;
    uint64_t s;           // splitmix64(seed)
    const int32_t *rowptr, *colidx;
    int32_t *rowptr_out, *colidx_out, *pos_out, *rowid_out;
    const int32_t *rows;  // [n_rows] the row list, or nullptr
    int32_t n_csr_rows, n_cols;
    uint8_t *col_mark;    // [n_cols] or nullptr: byte c becomes 1 for every kept entry of column c
    int32_t *range_flag;  // counters + 4: set by the scan kernels when the list holds an id outside [0, n_csr_rows)
};

__device__ __forceinline__ int32_t row_of(const Args &a, int32_t x) { return a.rows ? a.rows[x] : x; }

// ---- lengths and scan ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t kept_of(const Args &a, int64_t x)
{
    if (x >= a.n_rows) return 0;
    int32_t row = (int32_t)x;
    if (a.rows) {
        row = a.rows[x];
        if ((uint32_t)row >= (uint32_t)a.n_csr_rows) {   // refused on the host before anything is written
            atomicOr(a.range_flag, 1);
            return 0;
        }
    }
    const int32_t d = a.rowptr[row + 1] - a.rowptr[row];
    return d < 0 ? 0 : d < a.k ? d : a.k;   // (d < 0: a rowptr that gnnx_csr_validate would refuse)
}

// inclusive scan of one value per thread over the block of 256 (every thread calls it); total: the block's sum
__device__ __forceinline__ int32_t block_scan(int32_t v, int32_t *wave_sums, int32_t &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    __syncthreads();   // the sums of an earlier call have been read
    if (lane == 63) wave_sums[wv] = v;
    __syncthreads();
    int32_t before = 0;
    total = 0;
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const int32_t t = wave_sums[x];
        before += x < wv ? t : 0;
        total += t;
    }
    return v + before;
}

__global__ __launch_bounds__(256) void tile_sums_kernel(Args a, Lists w)
{
    __shared__ int32_t wave_sums[4];
    const int64_t row0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x;
    int32_t v = 0, total;
#pragma unroll
    for (int u = 0; u < kScanTile / 256; u++) v += kept_of(a, row0 + 256 * u);
    block_scan(v, wave_sums, total);
    if (threadIdx.x == 0) w.tile_sum[blockIdx.x] = total;
}

// one block: tile_sum becomes its exclusive scan, counters[2] the total
__global__ __launch_bounds__(256) void scan_tiles_kernel(Lists w)
{
    __shared__ int32_t wave_sums[4];
    int32_t carry = 0;
    for (int64_t base = 0; base < w.n_tiles; base += 256) {
        const int64_t i = base + threadIdx.x;
        const int32_t v = i < w.n_tiles ? w.tile_sum[i] : 0;
        int32_t total;
        const int32_t incl = block_scan(v, wave_sums, total);
        if (i < w.n_tiles) w.tile_sum[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) w.counters[2] = carry;
}

// rowptr_out[0 .. n_rows]: the rows of a tile scanned behind the tile's offset (row n_rows has length 0: it receives the total)
__global__ __launch_bounds__(256) void rowptr_kernel(Args a, Lists w)
{
    __shared__ int32_t wave_sums[4];
    int32_t carry = w.tile_sum[blockIdx.x];
#pragma unroll
    for (int u = 0; u < kScanTile / 256; u++) {
        const int64_t row = (int64_t)blockIdx.x * kScanTile + 256 * u + threadIdx.x;
        const int32_t v = kept_of(a, row);
        int32_t total;
        const int32_t incl = block_scan(v, wave_sums, total);
        if (row <= a.n_rows) a.rowptr_out[row] = carry + incl - v;
        carry += total;
    }
}

// ---- selection by a group of G lanes ---------------------------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ int32_t group_sum(int32_t v)
{
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the group's bits of a wavefront ballot, lane gbase at bit 0
template <int G>
__device__ __forceinline__ uint64_t group_ballot(bool pred, int gbase)
{
    const uint64_t m = __ballot(pred);
    return G == 64 ? m : (m >> gbase) & ((1ull << (G & 63)) - 1);
}

// The k-th smallest key of the items 0 .. n - 1 of `row` (item x has offset j_of(x); n > k >= 1), as a bound: exactly k items have a
// key <= the returned value.  Every lane of the group calls it and gets the same value.
template <int G, class JOf>
__device__ __forceinline__ uint64_t kth_key(uint64_t s, uint32_t row, int32_t n, int32_t k, int li, JOf j_of)
{
    uint64_t prefix = 0;       // the bits above `bit` of the k-th key
    int32_t cand = n;          // items that agree with prefix on those bits
    int32_t need = k;          // the k-th key is the need-th smallest of them; every item below the prefix is kept
    int bit = 64;
    while (cand != need && bit > 0) {
        bit--;
        const uint64_t mask = ~0ull << bit;
        int32_t zero = 0;      // candidates whose next bit is 0
        for (int32_t x = li; x < n; x += G) zero += (key_of(s, row, (uint32_t)j_of(x)) & mask) == prefix;
        zero = group_sum<G>(zero);
        if (zero >= need) {
            cand = zero;
        } else {
            need -= zero;
            cand -= zero;
            prefix |= 1ull << bit;
        }
    }
    return bit >= 64 ? ~0ull : prefix | ((1ull << bit) - 1);   // all the candidates left are kept
}

// emit(x_kept, j) for the items with a key <= bound, in ascending item order: x_kept counts them from 0 and stays below `limit`
template <int G, class JOf, class Emit>
__device__ __forceinline__ void keep_below(uint64_t s, uint32_t row, int32_t n, uint64_t bound, int32_t limit, int li, int gbase, JOf j_of,
                                           Emit emit)
{
    int32_t written = 0;
    for (int32_t base = 0; base < n; base += G) {
        const int32_t x = base + li;
        const int32_t j = x < n ? j_of(x) : 0;
        const bool keep = x < n && key_of(s, row, (uint32_t)j) <= bound;
        const uint64_t m = group_ballot<G>(keep, gbase);
        const int32_t at = written + __popcll(m & ((1ull << li) - 1));
        if (keep && at < limit) emit(at, j);
        written += __popcll(m);
    }
}

// kept entry q of output row x is entry j of its CSR row, which starts at b
__device__ __forceinline__ void store_entry(const Args &a, int32_t x, int64_t q, int64_t b, int32_t j)
{
    const int32_t col = a.colidx[b + j];
    a.colidx_out[q] = col;
    if (a.pos_out) a.pos_out[q] = (int32_t)(b + j);
    if (a.rowid_out) a.rowid_out[q] = x;
    if (a.col_mark && (uint32_t)col < (uint32_t)a.n_cols) a.col_mark[col] = 1;   // (many lanes storing the same 1 is the only race)
}

// 256 / G rows per block
template <int G>
__global__ __launch_bounds__(256) void rows_kernel(Args a, Lists w)
{
    const int li = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) - li;
    const int64_t row64 = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (row64 >= a.n_rows) return;                // uniform in the lane group; shuffles and ballots only ever meet lanes of the own group
    const int32_t x = (int32_t)row64;
    const int32_t row = row_of(a, x);
    const int64_t b = a.rowptr[row];
    const int64_t d = (int64_t)a.rowptr[row + 1] - b;
    const int64_t o = a.rowptr_out[x];
    if (d > kLong) {          // (L >= the largest k: such a row is never a copy)
        // Listed by one lane.  The lists are sized for rows met once each; a row list may repeat a long row more often than they
        // hold.  A row that found no slot is done right here by its lane group: slower, and the same entries.
        int32_t listed_it = 0;
        if (li == 0) {
            if (d > kSeg) {
                listed_it = append(w.hubs, x, d);
            } else {
                const int32_t at = atomicAdd(&w.counters[3], 1);
                listed_it = at < w.cap_long;   // holds on a valid CSR without a row list
                if (listed_it) w.long_rows[at] = x;
            }
        }
        if (__shfl(listed_it, gbase, 64)) return;
    }
    if (d <= a.k) {
        for (int32_t j = li; j < d; j += G) store_entry(a, x, o + j, b, j);
        return;
    }
    auto j_of = [](int32_t t) { return t; };
    const uint64_t bound = kth_key<G>(a.s, (uint32_t)row, (int32_t)d, a.k, li, j_of);
    keep_below<G>(a.s, (uint32_t)row, (int32_t)d, bound, a.k, li, gbase, j_of, [&](int32_t at, int32_t j) { store_entry(a, x, o + at, b, j); });
}

// a wavefront per listed row of L < d <= S entries
__global__ __launch_bounds__(256) void long_rows_kernel(Args a, Lists w)
{
    const int li = threadIdx.x & 63;
    const int64_t n_long = listed(&w.counters[3], w.cap_long);
    auto j_of = [](int32_t x) { return x; };
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_long; t += (int64_t)gridDim.x * 4) {
        const int32_t x = w.long_rows[t];
        const int32_t row = row_of(a, x);
        const int64_t b = a.rowptr[row];
        const int32_t d = (int32_t)(a.rowptr[row + 1] - b);
        const int64_t o = a.rowptr_out[x];
        const uint64_t bound = kth_key<64>(a.s, (uint32_t)row, d, a.k, li, j_of);
        keep_below<64>(a.s, (uint32_t)row, d, bound, a.k, li, 0, j_of, [&](int32_t at, int32_t j) { store_entry(a, x, o + at, b, j); });
    }
}

// a wavefront per segment slot: the offsets of the segment's min(k, len) smallest keys, ascending, to cand[slot, :]
__global__ __launch_bounds__(256) void seg_kernel(Args a, Lists w)
{
    const int li = threadIdx.x & 63;
    for_hub_segments(w.hubs, a.rowptr, a.rows, (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (int64_t)gridDim.x * 4,
                     [&](int32_t x, int32_t, int64_t s, int64_t, int64_t n, int64_t slot) {
        const int32_t row = row_of(a, x);
        const int32_t j0 = (int32_t)(s * kSeg), len = (int32_t)n;
        int32_t *out = w.cand + slot * a.k;
        auto j_of = [j0](int32_t x) { return j0 + x; };
        if (len <= a.k) {
            for (int32_t x = li; x < len; x += 64) out[x] = j0 + x;
            return;
        }
        const uint64_t bound = kth_key<64>(a.s, (uint32_t)row, len, a.k, li, j_of);
        keep_below<64>(a.s, (uint32_t)row, len, bound, a.k, li, 0, j_of, [&](int32_t at, int32_t j) { out[at] = j; });
    });
}

// a wavefront per hub: the k smallest of its candidates.  Every segment but the last holds exactly k (S > k), so the hub's candidates
// are the contiguous run cand[seg0 * k ...] of (nseg - 1) * k + min(k, last length) offsets in ascending order.
__global__ __launch_bounds__(256) void combine_kernel(Args a, Lists w)
{
    const int li = threadIdx.x & 63;
    const int64_t n_hubs = listed_hubs(w.hubs);
    for (int64_t h = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); h < n_hubs; h += (int64_t)gridDim.x * 4) {
        const int32_t x = w.hubs.hub_rows[h];
        if (x < 0) continue;
        const int32_t row = row_of(a, x);
        const int64_t b = a.rowptr[row];
        const int64_t d = (int64_t)a.rowptr[row + 1] - b;
        const int64_t o = a.rowptr_out[x];
        const int64_t nseg = (d + kSeg - 1) / kSeg;
        const int64_t last = d - (nseg - 1) * kSeg;
        const int32_t n = (int32_t)((nseg - 1) * a.k + (last < a.k ? last : a.k));   // > k: a hub has at least two segments
        const int32_t *cand = w.cand + (int64_t)w.hubs.hub_seg0[h] * a.k;
        auto j_of = [cand](int32_t x) { return cand[x]; };
        const uint64_t bound = kth_key<64>(a.s, (uint32_t)row, n, a.k, li, j_of);
        keep_below<64>(a.s, (uint32_t)row, n, bound, a.k, li, 0, j_of, [&](int32_t at, int32_t j) { store_entry(a, x, o + at, b, j); });
    }
}

template <int G>
int launch_rows(const Args &a, const Lists &w, hipStream_t st)
{
    hipLaunchKernelGGL(rows_kernel<G>, dim3((uint32_t)ceil_div(a.n_rows, 256 / G)), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    return GNNX_OK;
}

int check_sizes(int32_t n_rows, int64_t nnz, int32_t k)
{
    GNNX_REQUIRE(n_rows >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(k >= 1, GNNX_ERR_INVALID_ARG, "the fanout k must be at least 1, got %d", k);
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    return GNNX_OK;
}

// Both entry points.  n_out: rows of the output (n_csr_rows, or the list's length); the workspace is carved for (n_out, nnz, k) and the
// lane-group width comes from the CSR's mean row length.
int sample(int32_t n_csr_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_rows, int32_t n_out,
           int32_t k, uint64_t seed, int32_t *d_rowptr_out, int32_t *d_colidx_out, int32_t *d_pos_out, int32_t *d_rowid_out, uint8_t *d_col_mark,
           int64_t nnz_capacity, int64_t *nnz_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_sizes(n_csr_rows, nnz, k)) return rc;
    GNNX_REQUIRE(nnz_capacity >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(d_rowptr && d_rowptr_out && d_colidx_out && nnz_out && (d_colidx || nnz == 0), GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(k <= kMaxFanout, GNNX_ERR_UNSUPPORTED, "fanout %d: at most %d (one wavefront holds a row's selection)", k, kMaxFanout);
    Lists w;
    const size_t need = 256 + carve(n_out, nnz, k, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    *nnz_out = 0;
    hipStream_t st = as_stream(stream);
    if (n_out == 0) {   // a CSR of no rows: rowptr' = [0]
        GNNX_HIP_CHECK(hipMemsetAsync(d_rowptr_out, 0, sizeof(int32_t), st));
        GNNX_HIP_CHECK(hipStreamSynchronize(st));
        return GNNX_OK;
    }
    const Args a{n_out,  k,          splitmix64(seed), d_rowptr,   d_colidx,      d_rowptr_out, d_colidx_out, d_pos_out, d_rowid_out,
                 d_rows, n_csr_rows, n_cols,           d_col_mark, w.counters + 4};
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    hipLaunchKernelGGL(tile_sums_kernel, dim3((uint32_t)w.n_tiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(256), 0, st, w);
    GNNX_LAUNCH_CHECK();
    int32_t head[3] = {0, 0, 0};   // counters [2] the total, [3] (still 0), [4] the range flag
    GNNX_HIP_CHECK(hipMemcpyAsync(head, w.counters + 2, sizeof(head), hipMemcpyDeviceToHost, st));
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    GNNX_REQUIRE(!head[2], GNNX_ERR_INDEX_RANGE, "the row list holds an id outside [0, %d) (nothing was written)", n_csr_rows);
    const int32_t total = head[0];
    *nnz_out = total;   // also when the capacity is refused: what the caller has to offer
    GNNX_REQUIRE(total <= nnz_capacity, GNNX_ERR_INVALID_ARG, "the sample holds %d entries, nnz_capacity is %lld (nothing was written)", total,
                 (long long)nnz_capacity);
    hipLaunchKernelGGL(rowptr_kernel, dim3((uint32_t)w.n_tiles), dim3(256), 0, st, a, w);
    GNNX_LAUNCH_CHECK();
    if (total > 0) {
        const int64_t mean = nnz / n_csr_rows;   // lanes per row: how the rows map to lanes is not in the result
        int rc;
        if (mean > 32) rc = launch_rows<64>(a, w, st);
        else if (mean > 16) rc = launch_rows<32>(a, w, st);
        else if (mean > 8) rc = launch_rows<16>(a, w, st);
        else if (mean > 4) rc = launch_rows<8>(a, w, st);
        else rc = launch_rows<4>(a, w, st);
        if (rc) return rc;
        if (w.cap_long > 0) {   // nnz > L: a row can be longer than L
            hipLaunchKernelGGL(long_rows_kernel, dim3((uint32_t)ceil_div(w.cap_long < kSegWaves ? w.cap_long : kSegWaves, 4)), dim3(256), 0, st, a, w);
            GNNX_LAUNCH_CHECK();
        }
        const HubList &hubs = w.hubs;
        if (hubs.cap_hub > 0) {   // nnz > S: a row can be longer than S
            hipLaunchKernelGGL(seg_kernel, dim3((uint32_t)ceil_div(hubs.cap_seg < kSegWaves ? hubs.cap_seg : kSegWaves, 4)), dim3(256), 0, st, a, w);
            GNNX_LAUNCH_CHECK();
            hipLaunchKernelGGL(combine_kernel, dim3((uint32_t)ceil_div(hubs.cap_hub < kSegWaves ? hubs.cap_hub : kSegWaves, 4)), dim3(256), 0, st, a, w);
            GNNX_LAUNCH_CHECK();
        }
    }
    GNNX_HIP_CHECK(hipStreamSynchronize(st));
    return GNNX_OK;
}
}  // namespace

GNNX_API int gnnx_csr_sample_workspace(int32_t n_rows, int64_t nnz, int32_t k, size_t *bytes)
{
    GNNX_REQUIRE(bytes, GNNX_ERR_INVALID_ARG, "null pointer");
    if (int rc = check_sizes(n_rows, nnz, k)) return rc;
    GNNX_REQUIRE(k <= kMaxFanout, GNNX_ERR_UNSUPPORTED, "fanout %d: at most %d (one wavefront holds a row's selection)", k, kMaxFanout);
    *bytes = 256 + carve(n_rows, nnz, k, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_csr_sample_neighbors(int32_t n_rows, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, int32_t k, uint64_t seed,
                                       int32_t *d_rowptr_out, int32_t *d_colidx_out, int32_t *d_pos_out, int32_t *d_rowid_out,
                                       int64_t nnz_capacity, int64_t *nnz_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return sample(n_rows, 0, nnz, d_rowptr, d_colidx, nullptr, n_rows, k, seed, d_rowptr_out, d_colidx_out, d_pos_out, d_rowid_out, nullptr,
                  nnz_capacity, nnz_out, d_workspace, workspace_bytes, stream);
}

GNNX_API int gnnx_csr_sample_rows(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                  const int32_t *d_rows, int64_t n_listed, int32_t k, uint64_t seed, int32_t *d_rowptr_out, int32_t *d_colidx_out,
                                  int32_t *d_pos_out, int32_t *d_rowid_out, uint8_t *d_col_mark, int64_t nnz_capacity, int64_t *nnz_out,
                                  void *d_workspace, size_t workspace_bytes, void *stream)
{
    GNNX_REQUIRE(n_listed >= 0 && n_cols >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(n_listed < (1ll << 31), GNNX_ERR_INVALID_ARG, "the row list does not fit int32 output rows");
    GNNX_REQUIRE(d_rows || n_listed == 0, GNNX_ERR_INVALID_ARG, "null pointer");
    return sample(n_rows, n_cols, nnz, d_rowptr, d_colidx, d_rows, (int32_t)n_listed, k, seed, d_rowptr_out, d_colidx_out, d_pos_out, d_rowid_out,
                  d_col_mark, nnz_capacity, nnz_out, d_workspace, workspace_bytes, stream);   // (an empty list launches no kernel)
}
