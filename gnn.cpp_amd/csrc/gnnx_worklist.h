// The hub list of the units that cut a long CSR row into segments (gnnx_edge_softmax.hip, gnnx_reduce.hip, gnnx_sample.hip), once.
// A row of more than S = kSeg entries -- a hub -- is cut into ceil(d / S) segments of S consecutive entries (the last one shorter).
//   * listing: the unit's row kernel meets every row once; ONE lane per hub calls append(), which reserves the hub's slot h and its
//     run of segment slots s0 .. s0 + nseg - 1 with two counter atomics (never an atomic on a value) and writes hub_rows[h] = row,
//     hub_seg0[h] = s0 and seg_hub[slot] = h for every slot of the run;
//   * walking: later kernels of the same stream stride over the listed(counter, cap) slots with for_hub_segments(), which recovers
//     (row, segment, entries) from a slot, or over the listed hubs themselves (hub_rows[h], -1 skipped) to combine the segments'
//     partial results -- those live in the unit's own arrays, indexed by slot.
// The capacities are closed forms of (n_rows, nnz) that a workspace query evaluates on any host; a valid CSR never exceeds them.  On a
// broken one (rowptr not the prefix sums of its lengths) a hub that does not fit is marked -1 in both directions and skipped: no
// index ever leaves the arrays.  The counter words are zeroed on the stream in front of the row kernel of every call.  The order in
// which hubs land in the list varies from call to call; a unit's result must not depend on a row's slot.
#pragma once
#include "gnnx_common.h"

namespace gnnx {

constexpr int kSeg = 4096;   // S: the contract's segment length (include/gnnx.h)

// how many rows of more than `longer_than` entries a CSR of n_rows rows and nnz entries can hold
inline int64_t cap_rows_longer(int32_t n_rows, int64_t nnz, int64_t longer_than)
{
    const int64_t c = nnz / (longer_than + 1);
    return c < n_rows ? c : n_rows;
}

struct HubList {
    int32_t *counters;    // two words: [0] hubs listed, [1] segment slots handed out (either may pass its cap on a broken CSR)
    int32_t *hub_rows;    // [cap_hub]; -1: a hub whose segments did not fit (only a broken CSR can do that)
    int32_t *hub_seg0;    // [cap_hub] first slot of the hub's segments
    int32_t *seg_hub;     // [cap_seg] the hub (its slot in hub_rows) that a segment slot belongs to; -1: none
    int64_t cap_hub, cap_seg;

    void size(int32_t n_rows, int64_t nnz)
    {
        cap_hub = cap_rows_longer(n_rows, nnz, kSeg);
        cap_seg = nnz / kSeg + cap_hub;   // sum of ceil(d / S) <= nnz / S + hubs
    }
    // The arrays, packed as 4-byte words: the per-hub pair, then the per-slot array.  (Two calls because gnnx_edge_softmax.hip keeps
    // its per-head values between them; `two_counters`: the unit's zeroed words.)
    void take_hubs(Carver &c, int32_t *two_counters)
    {
        counters = two_counters;
        hub_rows = c.take<int32_t>((size_t)cap_hub, 4);
        hub_seg0 = c.take<int32_t>((size_t)cap_hub, 4);
    }
    void take_slots(Carver &c) { seg_hub = c.take<int32_t>((size_t)cap_seg, 4); }
};

// entries of a list whose counter may have run past its capacity
__device__ __forceinline__ int64_t listed(const int32_t *counter, int64_t cap)
{
    const int64_t n = *counter;
    return n < cap ? n : cap;
}
__device__ __forceinline__ int64_t listed_hubs(const HubList &w) { return listed(&w.counters[0], w.cap_hub); }

// one lane per hub row of d > S entries: its slot in the list and its run of segment slots.  Returns whether the hub was listed (always,
// on a valid CSR whose rows are met once each).  `row` is whatever the unit wants back from hub_rows[]: gnnx_sample.hip lists the
// position in its row list, which names the output row, and finds the CSR row through the list.
__device__ __forceinline__ bool append(const HubList &w, int32_t row, int64_t d)
{
    const int32_t nseg = (int32_t)((d + kSeg - 1) / kSeg);
    const int32_t h = atomicAdd(&w.counters[0], 1);
    const int32_t s0 = atomicAdd(&w.counters[1], nseg);
    const bool fits = h < w.cap_hub && (int64_t)s0 + nseg <= w.cap_seg;   // holds on a valid CSR
    if (h < w.cap_hub) {
        w.hub_rows[h] = fits ? row : -1;
        w.hub_seg0[h] = fits ? s0 : 0;
    }
    for (int64_t s = s0; s < (int64_t)s0 + nseg && s < w.cap_seg; s++) w.seg_hub[s] = fits ? h : -1;
    return fits;
}

// body(row, h, s, b, n, slot) for the slots first, first + stride, ... of the list: segment s of hub h, which is `row`, holds the n
// entries b .. b + n - 1 of the CSR.  The caller's work unit (a wavefront, a lane group) picks `first` and `stride`; every lane of the
// unit passes the same ones, so the body may shuffle.
// The overload with `rows` is for a hub list that holds positions in a row list: hub_rows[h] = x is handed to the body as it is, and
// the CSR row whose entries b .. b + n - 1 are meant is rows[x] (rows == nullptr: x itself).
template <class Body>
__device__ __forceinline__ void for_hub_segments(const HubList &w, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ rows, int64_t first,
                                                 int64_t stride, Body body)
{
    const int64_t n_slots = listed(&w.counters[1], w.cap_seg);
    for (int64_t slot = first; slot < n_slots; slot += stride) {
        const int32_t h = w.seg_hub[slot];
        if (h < 0) continue;
        const int32_t x = w.hub_rows[h];
        const int32_t row = rows ? rows[x] : x;
        const int64_t s = slot - w.hub_seg0[h];
        const int64_t row_end = rowptr[row + 1];
        const int64_t b = (int64_t)rowptr[row] + s * kSeg;
        const int64_t e = b + kSeg < row_end ? b + kSeg : row_end;
        body(x, h, s, b, e - b, slot);
    }
}
template <class Body>
__device__ __forceinline__ void for_hub_segments(const HubList &w, const int32_t *__restrict__ rowptr, int64_t first, int64_t stride, Body body)
{
    for_hub_segments(w, rowptr, nullptr, first, stride, body);
}

}  // namespace gnnx
