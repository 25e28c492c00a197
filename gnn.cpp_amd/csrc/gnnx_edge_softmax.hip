// Softmax over the stored entries of each CSR row, forward and backward -- include/gnnx.h "edge softmax".
//   t_p = (scores[p] + rowterm[i]) + colterm[c_p];  e_p = leaky_relu(t_p);  m_i = max_p e_p;  x_p = expf(e_p - m_i);
//   z_i = row sum of x_p;  alpha_p = x_p / z_i                                              for entry p of row i
// The ORDER of a row sum is part of the contract and a function of the row length d alone (the header states it): d <= S = 4096
// entries meet in G = min(64, pow2 >= d) virtual lanes (lane l adds entries l, l + G, ... ascending from +0, then the xor butterfly
// s = 1 .. G / 2); a longer row is cut into segments of S entries, each summed with G = 64, and the segment sums are added in
// ascending order.  How rows and segments map to wavefronts is NOT in the result:
//   * rows of d <= kShortW entries: kShortW lanes per row (64 / kShortW rows per wavefront), one entry per lane, everything in
//     registers -- the bulk of a power-law graph's rows.  The same kernel appends every longer row to one of two lists in the
//     caller's workspace (one global atomic per workgroup of 128 rows for the long rows, hubs are rare);
//   * long rows, kShortW < d <= S: a wavefront per listed row; up to 64 entries stay in registers, a longer row walks its entries
//     in three passes and parks e_p, then x_p, in d_out between them (each lane re-reads only what it stored itself): the column
//     term is gathered once;
//   * hub rows, d > S: a fixed grid strides over the segment slots of the hub list (gnnx_worklist.h); the maximum, the sum and the
//     division are separate launches because each needs the previous one complete for the whole row.  The segments' partial results
//     sit in the workspace and are combined in the fixed order by one lane per hub.
// Every launch is on the caller's stream and every ordering is a stream ordering; nothing is allocated or synchronised.  The
// order in which rows land in the lists varies from call to call, the values do not: a row's result never depends on its slot.
// Several heads (include/gnnx.h "multi-head attention"): every kernel takes the head from blockIdx.y and reads column h of the entry-major
// per-entry arrays; the lists are the pattern's and are written by head 0 only.  The single-head entry points launch one head.
#include "gnnx_worklist.h"

#pragma clang fp contract(off)

using namespace gnnx;

namespace {

constexpr int kShortW = 16;         // lanes per row of the short-row kernel
constexpr int kShortR = 8;          // rows per lane group of the short-row kernel
constexpr int kShortRowsPerBlock = (256 / kShortW) * kShortR;
constexpr int kLongWaves = 8192;    // wavefronts of the long-row kernel (grid stride over the list)
constexpr int kHubWaves = 4096;     // wavefronts of the hub kernels (stride over (hub, segment) pairs)
constexpr int kCounters = 16;       // int32 words in front of the workspace: [0], [1] the hub list's, [2] long rows

// the three operands of the pre-activation (each may be null, not all three) and the slope
struct Pre {
    const int32_t *colidx;
    const float *scores, *rowterm, *colterm;
    int64_t rs, cs;        // strides of the two terms
    int64_t ls;            // leading dimension of scores ([nnz, H] entry-major; 1 in the single-head calls)
    float slope;
};

// the caller's workspace, carved
struct Lists {
    int32_t *counters;      // kCounters words, zeroed by a memset on the stream in front of the first kernel
    int32_t *long_rows;     // [cap_long] rows of more than kShortW and at most S entries
    HubList hubs;
    float *hub_val;         // [H, cap_hub] the row's maximum, later its sum (forward); dot_i (backward)
    float *part;            // [H, cap_seg] one value per segment slot
    int64_t cap_long;
};

// the caller's pointer is taken as it is: the arrays are 4-byte words
size_t carve(int32_t n_rows, int64_t nnz, int32_t H, void *base, Lists *out)
{
    Lists w{};
    w.cap_long = cap_rows_longer(n_rows, nnz, kShortW);
    w.hubs.size(n_rows, nnz);
    Carver c(base);
    w.counters = c.take<int32_t>(kCounters, 4);
    w.long_rows = c.take<int32_t>((size_t)w.cap_long, 4);
    w.hubs.take_hubs(c, w.counters);
    w.hub_val = c.take<float>((size_t)w.hubs.cap_hub * H, 4);   // head h: hub_val + h cap_hub
    w.part = c.take<float>((size_t)w.hubs.cap_seg * H, 4);      //         part + h cap_seg
    w.hubs.take_slots(c);
    if (out) *out = w;
    return c.bytes();
}

// t_p = (scores[p] + rowterm[i]) + colterm[c_p], a null operand skipped; rt = rowterm[i * rs], loaded once per row
__device__ __forceinline__ float pre_activation(const Pre &a, int64_t p, float rt)
{
    float t = 0.f;
    if (a.scores) {
        t = a.scores[p * a.ls];
        if (a.rowterm) t = t + rt;
    } else if (a.rowterm) {
        t = rt;
    }
    if (a.colterm) {
        const float ct = a.colterm[(int64_t)a.colidx[p] * a.cs];
        t = (a.scores || a.rowterm) ? t + ct : ct;
    }
    return t;
}

__device__ __forceinline__ float leaky(float t, float slope) { return t > 0.f ? t : t * slope; }

// The head coordinate: blockIdx.y of every kernel below.  Head h reads column h of the entry-major per-entry arrays and element h of each
// term's row, and owns its own run of hub values and segment slots; the row lists (a function of the pattern alone) are shared and
// written by head 0 of the short-row kernel.  The single-head entry points are H = 1: every stride below is then 1 and head() adds 0.
__device__ __forceinline__ int head(Pre &a, Lists &w)
{
    const int h = blockIdx.y;
    if (a.scores) a.scores += h;
    if (a.rowterm) a.rowterm += h;
    if (a.colterm) a.colterm += h;
    w.hub_val += (int64_t)h * w.hubs.cap_hub;
    w.part += (int64_t)h * w.hubs.cap_seg;
    return h;
}

// f(k, t_p) for the entries k = l, l + 64, ... < n of a row piece whose first entry is b, in ascending k; the gathers of four entries
// are issued before the first is consumed (a lane's chain of dependent column-term loads is what a long row waits for)
template <class F>
__device__ __forceinline__ void for_lane_entries(const Pre &a, int64_t b, int64_t n, float rt, int l, F f)
{
    for (int64_t k0 = l; k0 < n; k0 += 4 * 64) {
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t k = k0 + 64 * j;
            t[j] = k < n ? pre_activation(a, b + k, rt) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t k = k0 + 64 * j;
            if (k < n) f(k, t[j]);
        }
    }
}

// G of a row or segment of d <= S entries: the smallest power of two >= d, capped at 64
__device__ __forceinline__ int lanes_of(int64_t d)
{
    int G = 1;
    while (G < d && G < 64) G <<= 1;
    return G;
}

// acc_l = acc_l + acc_{l xor s} for s = 1 .. G / 2 (G <= MAXG): every lane runs every shuffle, a stage with s >= G changes nothing.
// Partners stay inside the aligned group of G lanes, so lane groups with different G share a wavefront.
template <int MAXG>
__device__ __forceinline__ float add_lanes(float acc, int G)
{
#pragma unroll
    for (int s = 1; s < MAXG; s <<= 1) {
        const float o = __shfl_xor(acc, s, 64);
        if (s < G) acc = acc + o;
    }
    return acc;
}

template <int W>
__device__ __forceinline__ float max_lanes(float m)
{
#pragma unroll
    for (int s = 1; s < W; s <<= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    return m;
}

// Rows of one workgroup of the short-row kernels: 256 / kShortW lane groups, kShortR rows each; group g takes rows
// first + g, first + g + 16, ... so that neighbouring groups read neighbouring rowptr words.
struct ShortRows {
    int32_t row[kShortR];   // -1: behind the last row
    int32_t b[kShortR];     // the row's first entry
    int32_t d[kShortR];     // its length
};

__device__ __forceinline__ ShortRows load_short_rows(const int32_t *__restrict__ rowptr, int32_t n_rows)
{
    ShortRows r;
    const int64_t first = (int64_t)blockIdx.x * kShortRowsPerBlock + threadIdx.x / kShortW;
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        const int64_t row = first + j * (256 / kShortW);
        const bool in = row < n_rows;
        r.row[j] = in ? (int32_t)row : -1;
        r.b[j] = in ? rowptr[row] : 0;
        const int32_t d = in ? rowptr[row + 1] - r.b[j] : 0;
        r.d[j] = d < 0 ? 0 : d;
    }
    return r;
}

// Every row of the workgroup with more than kShortW entries goes to the lists.  Long rows: the workgroup counts them in LDS and
// reserves its run of slots with ONE global atomic (one per row, or per wavefront, serialises on the counter's address: a tenth of a
// power-law graph's rows are long).  Hubs are rare: each is appended to the hub list by its leader lane.
__device__ __forceinline__ void classify(const Lists &w, const ShortRows &r)
{
    __shared__ int32_t s_count, s_base;
    const bool leader = (threadIdx.x & (kShortW - 1)) == 0;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    int32_t slot[kShortR];
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        slot[j] = -1;
        if (!leader || r.d[j] <= kShortW) continue;
        if (r.d[j] <= kSeg) {
            slot[j] = atomicAdd(&s_count, 1);
            continue;
        }
        append(w.hubs, r.row[j], r.d[j]);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count > 0) s_base = atomicAdd(&w.counters[2], s_count);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        if (slot[j] < 0) continue;
        const int64_t at = (int64_t)s_base + slot[j];
        if (at < w.cap_long) w.long_rows[at] = r.row[j];   // the bound holds on a valid CSR
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// kShortW lanes per row, lane l holds entry l: e, x and the sum never leave registers.  The loads of a group's kShortR rows are all
// issued before the first is consumed.
__global__ __launch_bounds__(256) void fwd_short_kernel(int32_t n_rows, const int32_t *__restrict__ rowptr, Pre a, int unnorm,
                                                        float *__restrict__ out, int64_t ldo, float *__restrict__ rowmax,
                                                        float *__restrict__ rowsum, Lists w)
{
    const int hd = head(a, w), H = gridDim.y;
    out += hd;
    const int l = threadIdx.x & (kShortW - 1);
    const ShortRows r = load_short_rows(rowptr, n_rows);
    float e[kShortR];
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        e[j] = -INFINITY;
        if (r.d[j] <= kShortW && l < r.d[j]) {   // this kernel computes the row and this lane holds an entry
            const float rt = a.rowterm ? a.rowterm[(int64_t)r.row[j] * a.rs] : 0.f;
            e[j] = leaky(pre_activation(a, (int64_t)r.b[j] + l, rt), a.slope);
        }
    }
    if (hd == 0) classify(w, r);   // uniform in the workgroup
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        const bool own = r.row[j] >= 0 && r.d[j] <= kShortW;
        const bool have = own && l < r.d[j];
        const float m = max_lanes<kShortW>(e[j]);
        float acc = 0.f;
        float x = 0.f;
        if (have) {
            x = expf(e[j] - m);
            acc = acc + x;
        }
        const float z = add_lanes<kShortW>(acc, lanes_of(r.d[j]));
        if (have) out[((int64_t)r.b[j] + l) * ldo] = unnorm ? x : __fdiv_rn(x, z);
        if (own && l == 0) {
            if (rowmax) rowmax[(int64_t)r.row[j] * H + hd] = m;   // an empty row: -inf
            if (rowsum) rowsum[(int64_t)r.row[j] * H + hd] = z;   //               +0
        }
    }
}

// a wavefront per listed row of kShortW < d <= S entries
__global__ __launch_bounds__(256) void fwd_long_kernel(const int32_t *__restrict__ rowptr, Pre a, int unnorm, float *__restrict__ out,
                                                       int64_t ldo, float *__restrict__ rowmax, float *__restrict__ rowsum, Lists w)
{
    const int hd = head(a, w), H = gridDim.y;
    out += hd;
    const int l = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
    const int64_t n_long = listed(&w.counters[2], w.cap_long);
    for (int64_t i = wave; i < n_long; i += n_waves) {
        const int32_t row = w.long_rows[i];
        const int64_t b = rowptr[row], d = (int64_t)rowptr[row + 1] - b;
        const float rt = a.rowterm ? a.rowterm[(int64_t)row * a.rs] : 0.f;
        const int G = lanes_of(d);
        float m, z;
        if (d <= 64) {   // one entry per lane
            const bool have = l < d;
            const float e = have ? leaky(pre_activation(a, b + l, rt), a.slope) : -INFINITY;
            m = max_lanes<64>(e);
            float acc = 0.f, x = 0.f;
            if (have) {
                x = expf(e - m);
                acc = acc + x;
            }
            z = add_lanes<64>(acc, G);
            if (have) out[(b + l) * ldo] = unnorm ? x : __fdiv_rn(x, z);
        } else {         // G = 64: lane l owns entries l, l + 64, ...; e, then x, wait in out[] for the next pass
            m = -INFINITY;
            for_lane_entries(a, b, d, rt, l, [&](int64_t k, float t) {
                const float e = leaky(t, a.slope);
                out[(b + k) * ldo] = e;
                m = fmaxf(m, e);
            });
            m = max_lanes<64>(m);
            float acc = 0.f;
            for (int64_t k = l; k < d; k += 64) {
                const float x = expf(out[(b + k) * ldo] - m);
                out[(b + k) * ldo] = x;
                acc = acc + x;
            }
            z = add_lanes<64>(acc, 64);
            if (!unnorm)
                for (int64_t k = l; k < d; k += 64) out[(b + k) * ldo] = __fdiv_rn(out[(b + k) * ldo], z);
        }
        if (l == 0) {
            if (rowmax) rowmax[(int64_t)row * H + hd] = m;
            if (rowsum) rowsum[(int64_t)row * H + hd] = z;
        }
    }
}

// Hub passes: the wavefronts stride over the hub list's segment slots.  body(row, h, b, n, slot, l): the segment's first entry and
// length, its slot (of the head's `part`, too) and the lane.
template <class Body>
__device__ __forceinline__ void for_wave_segments(const int32_t *__restrict__ rowptr, const Lists &w, Body body)
{
    const int l = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
    for_hub_segments(w.hubs, rowptr, wave, n_waves,
                     [&](int32_t row, int32_t h, int64_t, int64_t b, int64_t n, int64_t slot) { body(row, h, b, n, slot, l); });
}

// e_p -> out, the segment's maximum -> part
__global__ __launch_bounds__(256) void fwd_hub_max_kernel(const int32_t *__restrict__ rowptr, Pre a, float *__restrict__ out, int64_t ldo,
                                                          Lists w)
{
    out += head(a, w);
    for_wave_segments(rowptr, w, [&](int32_t row, int32_t, int64_t b, int64_t n, int64_t slot, int l) {
        const float rt = a.rowterm ? a.rowterm[(int64_t)row * a.rs] : 0.f;
        float m = -INFINITY;
        for_lane_entries(a, b, n, rt, l, [&](int64_t k, float t) {
            const float e = leaky(t, a.slope);
            out[(b + k) * ldo] = e;
            m = fmaxf(m, e);
        });
        m = max_lanes<64>(m);
        if (l == 0) w.part[slot] = m;
    });
}

// a wavefront per hub: the maximum of its segments' maxima -> hub_val (and rowmax)
__global__ __launch_bounds__(256) void hub_combine_max_kernel(const int32_t *__restrict__ rowptr, float *__restrict__ rowmax, Lists w)
{
    Pre none{};
    const int hd = head(none, w), H = gridDim.y;
    const int l = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
    const int64_t n_hub = listed_hubs(w.hubs);
    for (int64_t h = wave; h < n_hub; h += n_waves) {
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)rowptr[row + 1] - rowptr[row] + kSeg - 1) / kSeg;
        const float *part = w.part + w.hubs.hub_seg0[h];
        float m = -INFINITY;
        for (int64_t s = l; s < nseg; s += 64) m = fmaxf(m, part[s]);
        m = max_lanes<64>(m);
        if (l == 0) {
            w.hub_val[h] = m;
            if (rowmax) rowmax[(int64_t)row * H + hd] = m;
        }
    }
}

// x_p = expf(e_p - m) -> out, the segment's sum (G = 64) -> part
__global__ __launch_bounds__(256) void fwd_hub_exp_kernel(const int32_t *__restrict__ rowptr, float *__restrict__ out, int64_t ldo, Lists w)
{
    Pre none{};
    out += head(none, w);
    for_wave_segments(rowptr, w, [&](int32_t, int32_t h, int64_t b, int64_t n, int64_t slot, int l) {
        const float m = w.hub_val[h];
        float acc = 0.f;
        for (int64_t k = l; k < n; k += 64) {
            const float x = expf(out[(b + k) * ldo] - m);
            out[(b + k) * ldo] = x;
            acc = acc + x;
        }
        acc = add_lanes<64>(acc, 64);
        if (l == 0) w.part[slot] = acc;
    });
}

// one lane per hub: ((seg_0 + seg_1) + seg_2) + ... -> hub_val and, when given, rows[row]
// rows: [n_rows] with stride ldr between rows, head h at element h
__global__ __launch_bounds__(256) void hub_combine_sum_kernel(const int32_t *__restrict__ rowptr, float *__restrict__ rows, int64_t ldr, Lists w)
{
    Pre none{};
    const int hd = head(none, w);
    const int64_t n_hub = listed_hubs(w.hubs);
    for (int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x; h < n_hub; h += (int64_t)gridDim.x * 256) {
        const int32_t row = w.hubs.hub_rows[h];
        if (row < 0) continue;
        const int64_t nseg = ((int64_t)rowptr[row + 1] - rowptr[row] + kSeg - 1) / kSeg;
        const float *part = w.part + w.hubs.hub_seg0[h];
        float z = part[0];
        for (int64_t s = 1; s < nseg; s++) z = z + part[s];
        w.hub_val[h] = z;
        if (rows) rows[(int64_t)row * ldr + hd] = z;
    }
}

// alpha_p = x_p / z
__global__ __launch_bounds__(256) void fwd_hub_div_kernel(const int32_t *__restrict__ rowptr, float *__restrict__ out, int64_t ldo, Lists w)
{
    Pre none{};
    out += head(none, w);
    for_wave_segments(rowptr, w, [&](int32_t, int32_t h, int64_t b, int64_t n, int64_t, int l) {
        const float z = w.hub_val[h];
        for (int64_t k = l; k < n; k += 64) out[(b + k) * ldo] = __fdiv_rn(out[(b + k) * ldo], z);
    });
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// dt_p of one entry from the row's dot_i
__device__ __forceinline__ float dt_of(float t, float slope, float al, float da, float dot)
{
    const float de = al * (da - dot);
    return t > 0.f ? de : de * slope;
}

// the backward's per-entry arrays with their leading dimensions, and the stride between two rows of drowterm
struct Bwd {
    const float *alpha;
    int64_t lda;
    const float *dalpha;
    int64_t ldd;
    float *dt;
    int64_t ldt;
    float *drowterm;
    int64_t drs;
};

__device__ __forceinline__ void head(Bwd &g, int h)
{
    g.alpha += h;
    g.dalpha += h;
    g.dt += h;
    if (g.drowterm) g.drowterm += h;
}

__global__ __launch_bounds__(256) void bwd_short_kernel(int32_t n_rows, const int32_t *__restrict__ rowptr, Pre a, Bwd g, Lists w)
{
    const int hd = head(a, w);
    head(g, hd);
    const int l = threadIdx.x & (kShortW - 1);
    const ShortRows r = load_short_rows(rowptr, n_rows);
    float al[kShortR], da[kShortR], t[kShortR];
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        al[j] = da[j] = t[j] = 0.f;
        if (r.d[j] <= kShortW && l < r.d[j]) {
            const int64_t p = (int64_t)r.b[j] + l;
            const float rt = a.rowterm ? a.rowterm[(int64_t)r.row[j] * a.rs] : 0.f;
            al[j] = g.alpha[p * g.lda];
            da[j] = g.dalpha[p * g.ldd];
            t[j] = pre_activation(a, p, rt);
        }
    }
    if (hd == 0) classify(w, r);   // uniform in the workgroup
#pragma unroll
    for (int j = 0; j < kShortR; j++) {
        const bool own = r.row[j] >= 0 && r.d[j] <= kShortW;
        const bool have = own && l < r.d[j];
        const int G = lanes_of(r.d[j]);
        float acc = 0.f;
        if (have) acc = acc + (al[j] * da[j]);
        const float dot = add_lanes<kShortW>(acc, G);
        acc = 0.f;
        if (have) {
            const float de = al[j] * (da[j] - dot);
            const float v = t[j] > 0.f ? de : de * a.slope;
            g.dt[((int64_t)r.b[j] + l) * g.ldt] = v;
            acc = acc + v;
        }
        const float sum = add_lanes<kShortW>(acc, G);
        if (own && l == 0 && g.drowterm) g.drowterm[(int64_t)r.row[j] * g.drs] = sum;   // an empty row: +0
    }
}

__global__ __launch_bounds__(256) void bwd_long_kernel(const int32_t *__restrict__ rowptr, Pre a, Bwd g, Lists w)
{
    head(g, head(a, w));
    const int l = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
    const int64_t n_long = listed(&w.counters[2], w.cap_long);
    for (int64_t i = wave; i < n_long; i += n_waves) {
        const int32_t row = w.long_rows[i];
        const int64_t b = rowptr[row], d = (int64_t)rowptr[row + 1] - b;
        const float rt = a.rowterm ? a.rowterm[(int64_t)row * a.rs] : 0.f;
        const int G = lanes_of(d);
        float sum;
        if (d <= 64) {
            const bool have = l < d;
            float al = 0.f, da = 0.f, acc = 0.f;
            if (have) {
                al = g.alpha[(b + l) * g.lda];
                da = g.dalpha[(b + l) * g.ldd];
                acc = acc + (al * da);
            }
            const float dot = add_lanes<64>(acc, G);
            acc = 0.f;
            if (have) {
                const float v = dt_of(pre_activation(a, b + l, rt), a.slope, al, da, dot);
                g.dt[(b + l) * g.ldt] = v;
                acc = acc + v;
            }
            sum = add_lanes<64>(acc, G);
        } else {
            float acc = 0.f;
            for (int64_t k = l; k < d; k += 64) acc = acc + (g.alpha[(b + k) * g.lda] * g.dalpha[(b + k) * g.ldd]);
            const float dot = add_lanes<64>(acc, 64);
            acc = 0.f;
            for_lane_entries(a, b, d, rt, l, [&](int64_t k, float t) {
                const float v = dt_of(t, a.slope, g.alpha[(b + k) * g.lda], g.dalpha[(b + k) * g.ldd], dot);
                g.dt[(b + k) * g.ldt] = v;
                acc = acc + v;
            });
            sum = add_lanes<64>(acc, 64);
        }
        if (l == 0 && g.drowterm) g.drowterm[(int64_t)row * g.drs] = sum;
    }
}

// the segment's sum of w_p = alpha_p * dalpha_p -> part
__global__ __launch_bounds__(256) void bwd_hub_dot_kernel(const int32_t *__restrict__ rowptr, Bwd g, Lists w)
{
    Pre none{};
    head(g, head(none, w));
    for_wave_segments(rowptr, w, [&](int32_t, int32_t, int64_t b, int64_t n, int64_t slot, int l) {
        float acc = 0.f;
        for (int64_t k = l; k < n; k += 64) acc = acc + (g.alpha[(b + k) * g.lda] * g.dalpha[(b + k) * g.ldd]);
        acc = add_lanes<64>(acc, 64);
        if (l == 0) w.part[slot] = acc;
    });
}

// dt_p -> dt, the segment's sum of dt_p -> part
__global__ __launch_bounds__(256) void bwd_hub_dt_kernel(const int32_t *__restrict__ rowptr, Pre a, Bwd g, Lists w)
{
    head(g, head(a, w));
    for_wave_segments(rowptr, w, [&](int32_t row, int32_t h, int64_t b, int64_t n, int64_t slot, int l) {
        const float rt = a.rowterm ? a.rowterm[(int64_t)row * a.rs] : 0.f;
        const float dot = w.hub_val[h];
        float acc = 0.f;
        for_lane_entries(a, b, n, rt, l, [&](int64_t k, float t) {
            const float v = dt_of(t, a.slope, g.alpha[(b + k) * g.lda], g.dalpha[(b + k) * g.ldd], dot);
            g.dt[(b + k) * g.ldt] = v;
            acc = acc + v;
        });
        acc = add_lanes<64>(acc, 64);
        if (l == 0) w.part[slot] = acc;
    });
}

inline uint32_t blocks_for_waves(int64_t waves, int64_t cap) { return (uint32_t)ceil_div(waves < cap ? waves : cap, 4); }

// what every entry point checks before any device call
int check_args(int32_t n_rows, int32_t n_cols, int64_t nnz, int32_t n_heads, const int32_t *d_rowptr, const int32_t *d_colidx,
               const float *d_scores, int64_t lds, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm,
               int64_t colterm_stride)
{
    GNNX_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GNNX_ERR_INVALID_ARG, "negative size");
    GNNX_REQUIRE(nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "nnz does not fit the int32 CSR");
    GNNX_REQUIRE(n_heads >= 1 && n_heads < 65536, GNNX_ERR_INVALID_ARG, "n_heads outside [1, 65535]");
    GNNX_REQUIRE(d_scores || d_rowterm || d_colterm, GNNX_ERR_INVALID_ARG, "scores, rowterm and colterm are all null");
    GNNX_REQUIRE(!d_scores || lds >= n_heads, GNNX_ERR_INVALID_ARG, "leading dimension of scores < n_heads");
    GNNX_REQUIRE((!d_rowterm || rowterm_stride >= n_heads) && (!d_colterm || colterm_stride >= n_heads), GNNX_ERR_INVALID_ARG,
                 "term stride < %d", n_heads);
    GNNX_REQUIRE(d_rowptr, GNNX_ERR_INVALID_ARG, "null pointer");
    GNNX_REQUIRE(nnz == 0 || (n_rows > 0 && n_cols > 0), GNNX_ERR_INVALID_ARG, "entries in a matrix without rows or columns");
    GNNX_REQUIRE(nnz == 0 || d_colidx, GNNX_ERR_INVALID_ARG, "null pointer");
    return GNNX_OK;
}

int forward(int32_t n_rows, int32_t n_cols, int64_t nnz, int32_t H, const int32_t *d_rowptr, const int32_t *d_colidx, const float *d_scores,
            int64_t lds, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm, int64_t colterm_stride, float negative_slope,
            uint32_t flags, float *d_out, int64_t ldo, float *d_rowmax, float *d_rowsum, void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_args(n_rows, n_cols, nnz, H, d_rowptr, d_colidx, d_scores, lds, d_rowterm, rowterm_stride, d_colterm, colterm_stride);
    if (rc) return rc;
    GNNX_REQUIRE(!(flags & ~(uint32_t)GNNX_EDGE_SOFTMAX_UNNORMALISED), GNNX_ERR_INVALID_ARG, "unknown flag");
    GNNX_REQUIRE(ldo >= H, GNNX_ERR_INVALID_ARG, "leading dimension of out < n_heads");
    GNNX_REQUIRE(nnz == 0 || d_out, GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Lists w;
    const size_t need = carve(n_rows, nnz, H, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const Pre a{d_colidx, d_scores, d_rowterm, d_colterm, rowterm_stride, colterm_stride, lds, negative_slope};
    const int unnorm = (flags & GNNX_EDGE_SOFTMAX_UNNORMALISED) ? 1 : 0;
    const uint32_t Hy = (uint32_t)H;
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    hipLaunchKernelGGL(fwd_short_kernel, dim3((uint32_t)ceil_div(n_rows, kShortRowsPerBlock), Hy), dim3(256), 0, st, n_rows, d_rowptr, a, unnorm,
                       d_out, ldo, d_rowmax, d_rowsum, w);
    GNNX_LAUNCH_CHECK();
    if (w.cap_long > 0) {
        hipLaunchKernelGGL(fwd_long_kernel, dim3(blocks_for_waves(w.cap_long, kLongWaves), Hy), dim3(256), 0, st, d_rowptr, a, unnorm, d_out, ldo,
                           d_rowmax, d_rowsum, w);
        GNNX_LAUNCH_CHECK();
    }
    if (w.hubs.cap_hub > 0) {
        const dim3 seg_grid(blocks_for_waves(w.hubs.cap_seg, kHubWaves), Hy), hub_grid(blocks_for_waves(w.hubs.cap_hub, 1024), Hy);
        hipLaunchKernelGGL(fwd_hub_max_kernel, seg_grid, dim3(256), 0, st, d_rowptr, a, d_out, ldo, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(hub_combine_max_kernel, hub_grid, dim3(256), 0, st, d_rowptr, d_rowmax, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(fwd_hub_exp_kernel, seg_grid, dim3(256), 0, st, d_rowptr, d_out, ldo, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(hub_combine_sum_kernel, dim3((uint32_t)ceil_div(w.hubs.cap_hub < 65536 ? w.hubs.cap_hub : 65536, 256), Hy), dim3(256), 0, st,
                           d_rowptr, d_rowsum, (int64_t)H, w);
        GNNX_LAUNCH_CHECK();
        if (!unnorm) {
            hipLaunchKernelGGL(fwd_hub_div_kernel, seg_grid, dim3(256), 0, st, d_rowptr, d_out, ldo, w);
            GNNX_LAUNCH_CHECK();
        }
    }
    return GNNX_OK;
}

int backward(int32_t n_rows, int32_t n_cols, int64_t nnz, int32_t H, const int32_t *d_rowptr, const int32_t *d_colidx, const float *d_scores,
             int64_t lds, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm, int64_t colterm_stride, float negative_slope,
             const Bwd &g, void *d_workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_args(n_rows, n_cols, nnz, H, d_rowptr, d_colidx, d_scores, lds, d_rowterm, rowterm_stride, d_colterm, colterm_stride);
    if (rc) return rc;
    GNNX_REQUIRE(g.lda >= H && g.ldd >= H && g.ldt >= H && (!g.drowterm || g.drs >= H), GNNX_ERR_INVALID_ARG,
                 "a leading dimension or the drowterm stride < n_heads");
    GNNX_REQUIRE(nnz == 0 || (g.alpha && g.dalpha && g.dt), GNNX_ERR_INVALID_ARG, "null pointer");
    if (n_rows == 0) return GNNX_OK;
    Lists w;
    const size_t need = carve(n_rows, nnz, H, d_workspace, &w);
    GNNX_REQUIRE(d_workspace && workspace_bytes >= need, GNNX_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const Pre a{d_colidx, d_scores, d_rowterm, d_colterm, rowterm_stride, colterm_stride, lds, negative_slope};
    const uint32_t Hy = (uint32_t)H;
    GNNX_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(int32_t) * kCounters, st));
    hipLaunchKernelGGL(bwd_short_kernel, dim3((uint32_t)ceil_div(n_rows, kShortRowsPerBlock), Hy), dim3(256), 0, st, n_rows, d_rowptr, a, g, w);
    GNNX_LAUNCH_CHECK();
    if (w.cap_long > 0) {
        hipLaunchKernelGGL(bwd_long_kernel, dim3(blocks_for_waves(w.cap_long, kLongWaves), Hy), dim3(256), 0, st, d_rowptr, a, g, w);
        GNNX_LAUNCH_CHECK();
    }
    if (w.hubs.cap_hub > 0) {
        const dim3 seg_grid(blocks_for_waves(w.hubs.cap_seg, kHubWaves), Hy);
        const dim3 lane_grid((uint32_t)ceil_div(w.hubs.cap_hub < 65536 ? w.hubs.cap_hub : 65536, 256), Hy);
        hipLaunchKernelGGL(bwd_hub_dot_kernel, seg_grid, dim3(256), 0, st, d_rowptr, g, w);
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(hub_combine_sum_kernel, lane_grid, dim3(256), 0, st, d_rowptr, (float *)nullptr, (int64_t)0, w);   // dot_i -> hub_val
        GNNX_LAUNCH_CHECK();
        hipLaunchKernelGGL(bwd_hub_dt_kernel, seg_grid, dim3(256), 0, st, d_rowptr, a, g, w);
        GNNX_LAUNCH_CHECK();
        if (g.drowterm) {
            hipLaunchKernelGGL(hub_combine_sum_kernel, lane_grid, dim3(256), 0, st, d_rowptr, g.drowterm, g.drs, w);
            GNNX_LAUNCH_CHECK();
        }
    }
    return GNNX_OK;
}

}  // namespace

GNNX_API int gnnx_edge_softmax_workspace(int32_t n_rows, int64_t nnz, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_rows >= 0 && nnz >= 0 && nnz < (1ll << 31), GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = carve(n_rows, nnz, 1, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_edge_softmax_heads_workspace(int32_t n_rows, int64_t nnz, int32_t n_heads, size_t *bytes)
{
    GNNX_REQUIRE(bytes && n_rows >= 0 && nnz >= 0 && nnz < (1ll << 31) && n_heads >= 1 && n_heads < 65536, GNNX_ERR_INVALID_ARG, "bad arguments");
    *bytes = carve(n_rows, nnz, n_heads, nullptr, nullptr);
    return GNNX_OK;
}

GNNX_API int gnnx_edge_softmax_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                       const float *d_scores, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm,
                                       int64_t colterm_stride, float negative_slope, uint32_t flags, float *d_out, float *d_rowmax,
                                       float *d_rowsum, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return forward(n_rows, n_cols, nnz, 1, d_rowptr, d_colidx, d_scores, 1, d_rowterm, rowterm_stride, d_colterm, colterm_stride, negative_slope,
                   flags, d_out, 1, d_rowmax, d_rowsum, d_workspace, workspace_bytes, stream);
}

GNNX_API int gnnx_edge_softmax_csr_heads_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                             int32_t n_heads, const float *d_scores, int64_t lds, const float *d_rowterm, int64_t rowterm_stride,
                                             const float *d_colterm, int64_t colterm_stride, float negative_slope, uint32_t flags, float *d_out,
                                             int64_t ldo, float *d_rowmax, float *d_rowsum, void *d_workspace, size_t workspace_bytes,
                                             void *stream)
{
    return forward(n_rows, n_cols, nnz, n_heads, d_rowptr, d_colidx, d_scores, lds, d_rowterm, rowterm_stride, d_colterm, colterm_stride,
                   negative_slope, flags, d_out, ldo, d_rowmax, d_rowsum, d_workspace, workspace_bytes, stream);
}

GNNX_API int gnnx_edge_softmax_bwd_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                           const float *d_scores, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm,
                                           int64_t colterm_stride, float negative_slope, const float *d_alpha, const float *d_dalpha,
                                           float *d_dt, float *d_drowterm, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const Bwd g{d_alpha, 1, d_dalpha, 1, d_dt, 1, d_drowterm, 1};
    return backward(n_rows, n_cols, nnz, 1, d_rowptr, d_colidx, d_scores, 1, d_rowterm, rowterm_stride, d_colterm, colterm_stride, negative_slope,
                    g, d_workspace, workspace_bytes, stream);
}

GNNX_API int gnnx_edge_softmax_bwd_csr_heads_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                                 int32_t n_heads, const float *d_scores, int64_t lds, const float *d_rowterm,
                                                 int64_t rowterm_stride, const float *d_colterm, int64_t colterm_stride, float negative_slope,
                                                 const float *d_alpha, int64_t lda, const float *d_dalpha, int64_t ldd, float *d_dt, int64_t ldt,
                                                 float *d_drowterm, int64_t drowterm_stride, void *d_workspace, size_t workspace_bytes,
                                                 void *stream)
{
    const Bwd g{d_alpha, lda, d_dalpha, ldd, d_dt, ldt, d_drowterm, drowterm_stride};
    return backward(n_rows, n_cols, nnz, n_heads, d_rowptr, d_colidx, d_scores, lds, d_rowterm, rowterm_stride, d_colterm, colterm_stride,
                    negative_slope, g, d_workspace, workspace_bytes, stream);
}
