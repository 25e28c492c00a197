"""A plain restatement of the 1-D vertex partition and the halo plan behind the C-ABI (gnn.cpp_amd/csrc/gnnx_shard.hip:
gnnx_vertex_weights, gnnx_partition_deal, gnnx_partition_scramble, gnnx_shard_select_edges, gnnx_halo_plan_create,
gnnx_halo_plan_set_send_list, gnnx_halo_plan_info, gnnx_halo_plan_slot_table) and the case list of tests/test_gpu_shard_plan.py.

Written from the contract in include/gnnx.h (section "partition + halo plan"), one function per call, in NumPy and plain Python
loops: no torch, no sort / scan primitives shared with the kernels or with gnn.cpp_amd/shard.py.  tests/test_shard_ref_cpu.py pins
it to hand-written expectations and to shard.py on CPU torch, and shows that the case list can tell a wrong answer from a right
one.  Everything here is integer work: every comparison against it is equality."""
import numpy as np

SCRAMBLE_MUL = 2654435761   # include/gnnx.h, gnnx_partition_scramble
SLOTS = 8                   # columns of the slot table; a row may fill at most SLOTS - 1 of them


# ------------------------------------------------------------------ partition
def vertex_weights(src, dst, n, row_weight):
    """w[v] = out-degree + in-degree + row_weight; self loops and duplicates count as given.  ValueError on an endpoint outside
    [0, n)."""
    w = [int(row_weight)] * int(n)
    for r, c in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if not (0 <= r < n and 0 <= c < n):
            raise ValueError("edge endpoint outside [0, n)")
        w[r] += 1
        w[c] += 1
    return np.array(w, dtype=np.int32).reshape(-1)


def deal_order(weight):
    """Vertices in descending weight, ties by ascending id."""
    w = [int(x) for x in np.asarray(weight).tolist()]
    return sorted(range(len(w)), key=lambda v: (-w[v], v))


def snake_rank(k, world):
    """Rank of position k of the order: k % world in even rounds k // world, world - 1 - k % world in odd rounds."""
    j, r = k % world, k // world
    return j if r % 2 == 0 else world - 1 - j


def deal_from(order, rank_of_position, world):
    """(owner, nid, cuts) of a deal: position k of `order` goes to rank_of_position(k, world); nid numbers rank p's vertices
    cuts[p].. in ascending original id."""
    n = len(order)
    owner = [0] * n
    for k, v in enumerate(order):
        owner[v] = rank_of_position(k, world)
    cuts = [0]
    for p in range(world):
        cuts.append(cuts[-1] + sum(1 for v in range(n) if owner[v] == p))
    nxt = list(cuts[:-1])
    nid = [0] * n
    for v in range(n):                      # ascending original id
        nid[v] = nxt[owner[v]]
        nxt[owner[v]] += 1
    return np.array(owner, dtype=np.int32).reshape(-1), np.array(nid, dtype=np.int32).reshape(-1), cuts


def deal(weight, world):
    """gnnx_partition_deal: (owner int32 [n], nid int32 [n], cuts list [world + 1]).  world == 1 is the identity, n == 0 gives
    all-zero cuts."""
    assert world >= 1
    return deal_from(deal_order(weight), snake_rank, world)


def scramble(owner, nid, cuts):
    """gnnx_partition_scramble: position k of rank p's n_p rows moves to (k * SCRAMBLE_MUL) % n_p (Python integers)."""
    out = []
    for p, x in zip(np.asarray(owner).tolist(), np.asarray(nid).tolist()):
        lo, n_p = cuts[p], cuts[p + 1] - cuts[p]
        out.append(lo + ((x - lo) * SCRAMBLE_MUL) % n_p)
    return np.array(out, dtype=np.int32).reshape(-1)


def partition(src, dst, n, world, row_weight):
    """weights -> deal -> scramble, as every caller chains them: (weight, owner, nid before the scramble, nid, cuts)."""
    w = vertex_weights(src, dst, n, row_weight)
    owner, nid0, cuts = deal(w, world)
    return w, owner, nid0, scramble(owner, nid0, cuts), cuts


# ------------------------------------------------------------------ a rank's edges
def select_edges(src, dst, owner, nid, rank, lo, transpose):
    """gnnx_shard_select_edges: (rows int32, cols int32) of the edges rank `rank` owns, in original edge order.  Self loops are
    dropped on original ids; rows = nid - lo of the owned endpoint, cols = the ORIGINAL id of the other one."""
    rows, cols = [], []
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if s == d:
            continue
        r, c = (d, s) if transpose else (s, d)
        if int(owner[r]) == rank:
            rows.append(int(nid[r]) - lo)
            cols.append(c)
    return np.array(rows, dtype=np.int32).reshape(-1), np.array(cols, dtype=np.int32).reshape(-1)


def shard_csr(rows, cols, n_local):
    """(rowptr int64 [n_local + 1], colidx int32) of the selection: sorted by (row, original column), duplicates collapsed (what
    gnnx_csr_from_coo with GNNX_CSR_KEEP_SELF_LOOPS builds from it; that builder is held to tests/graph_ref.py by its own tests)."""
    pairs = sorted(set(zip(np.asarray(rows).tolist(), np.asarray(cols).tolist())))
    rowptr = [0] * (n_local + 1)
    for r, _ in pairs:
        rowptr[r + 1] += 1
    for r in range(n_local):
        rowptr[r + 1] += rowptr[r]
    return np.array(rowptr, dtype=np.int64), np.array([c for _, c in pairs], dtype=np.int32).reshape(-1)


# ------------------------------------------------------------------ halo plan
def halo_plan(colidx_orig, nid, cuts, rank):
    """gnnx_halo_plan_create: (halo int32 [n_halo], colidx_local int32 [nnz], recv_rows list [world]).  halo = the sorted new ids of
    the remote columns; a local column c (new id) becomes c - lo, a remote one n_local + its position in halo; entry order
    untouched; recv_rows[q] = halo rows owned by q."""
    world = len(cuts) - 1
    lo, hi = cuts[rank], cuts[rank + 1]
    new = [int(nid[c]) for c in np.asarray(colidx_orig).tolist()]
    halo = sorted({c for c in new if not lo <= c < hi})
    where = {c: i for i, c in enumerate(halo)}
    local = [c - lo if lo <= c < hi else (hi - lo) + where[c] for c in new]
    recv = [sum(1 for c in halo if cuts[q] <= c < cuts[q + 1]) for q in range(world)]
    return np.array(halo, dtype=np.int32).reshape(-1), np.array(local, dtype=np.int32).reshape(-1), recv


def send_lists(halos, cuts):
    """What the requests deliver to every owner p (gnnx_halo_plan_exchange_requests / gnnx_halo_plan_set_send_list), from the halo
    lists of ALL ranks: a list over p of (want_p, send_rows_p, send_idx_p).  want_p = the concatenation over the peers q, in rank
    order, of halo_q within [cuts[p], cuts[p+1]); send_rows_p the matching counts; send_idx_p = want_p - cuts[p]."""
    world = len(cuts) - 1
    out = []
    for p in range(world):
        want, counts = [], []
        for q in range(world):
            part = [int(c) for c in np.asarray(halos[q]).tolist() if cuts[p] <= c < cuts[p + 1]]
            want += part
            counts.append(len(part))
        out.append((np.array(want, dtype=np.int32).reshape(-1), counts, np.array([c - cuts[p] for c in want], dtype=np.int32).reshape(-1)))
    return out


def slot_table(send_idx, n_local):
    """gnnx_halo_plan_slot_table: [n_local, 8] int32, row r's positions in the send list (send_idx[slot] == r) ascending, packed to
    the front, -1 behind; None when some row has more than 7 slots."""
    table = np.full((n_local, SLOTS), -1, dtype=np.int32)
    fill = [0] * n_local
    for slot, r in enumerate(np.asarray(send_idx).tolist()):
        if fill[r] == SLOTS - 1:
            return None
        table[r, fill[r]] = slot
        fill[r] += 1
    return table


def inverse(nid):
    """orig[new id] = original id."""
    orig = np.empty(len(nid), dtype=np.int64)
    orig[np.asarray(nid, dtype=np.int64)] = np.arange(len(nid))
    return orig


# ------------------------------------------------------------------ the case list
WORLDS = (1, 2, 3, 8, 9)
ROW_WEIGHTS = (0, 3)
STAR_N, STAR_HUB = 40, 17


def _i32(x):
    return np.array(x, dtype=np.int32).reshape(-1)


def graph(name, synth=None):
    """(src int32, dst int32, n) of a named case; every one is tiny and chosen for one edge of the index code."""
    if name == "empty":         # the early returns; cuts all zero
        return _i32([]), _i32([]), 0
    if name == "lonely1":       # no edges: weights equal row_weight, no halo, nothing selected
        return _i32([]), _i32([]), 1
    if name == "lonely5":
        return _i32([]), _i32([]), 5
    if name == "loops":         # only self loops, some twice: every edge dropped, plans made with nnz == 0
        return _i32([0, 3, 3, 4, 1, 3]), _i32([0, 3, 3, 4, 1, 3]), 5
    if name == "order":         # unsorted, duplicates, one self loop: the selection keeps edge order
        return _i32([4, 0, 5, 2, 4, 1, 3, 0, 5, 2, 4]), _i32([1, 3, 0, 2, 1, 5, 4, 3, 2, 0, 0]), 6
    if name == "ring257":       # all weights tied: id order alone decides; n crosses one 256-thread block
        v = np.arange(257)
        return _i32(v), _i32((v + 1) % 257), 257
    if name == "star":          # one heavy vertex whose row every other rank reads
        v = np.array([x for x in range(STAR_N) if x != STAR_HUB])
        hub = np.full(v.size, STAR_HUB)
        return _i32(np.concatenate([v, hub])), _i32(np.concatenate([hub, v])), STAR_N
    if name == "rmat":          # several blocks of vertices and edges, many ties, empty rows, duplicates
        s, d = synth.rmat_edges(31, 1000, 8000)
        return _i32(s), _i32(d), 1000
    if name == "few":           # with world 8: ranks without rows, repeated cuts, n_local == 0 plans
        return _i32([0, 1, 2, 2]), _i32([1, 2, 0, 1]), 3
    raise KeyError(name)


def combinations():
    """(graph name, world, row_weight) of every case: the graphs crossed with WORLDS and ROW_WEIGHTS; `few` needs only world 8,
    `empty` only worlds 1 and 3."""
    out = []
    for name in ("empty", "lonely1", "lonely5", "loops", "order", "ring257", "star", "rmat", "few"):
        worlds = (8,) if name == "few" else (1, 3) if name == "empty" else WORLDS
        out += [(name, w, rw) for w in worlds for rw in ROW_WEIGHTS]
    return out


class Plan:
    """The whole restated plan of one (graph, world, row_weight): partition, then for both transpositions and every rank the
    selection, its CSR, the halo plan, and the send lists / slot tables of every owner."""

    def __init__(self, src, dst, n, world, row_weight):
        self.src, self.dst, self.n, self.world = src, dst, n, world
        self.weight, self.owner, self.nid0, self.nid, self.cuts = partition(src, dst, n, world, row_weight)
        self.orig = inverse(self.nid)
        self.sides = {}
        for transpose in (False, True):
            ranks = []
            for rank in range(world):
                lo, hi = self.cuts[rank], self.cuts[rank + 1]
                rows, cols = select_edges(src, dst, self.owner, self.nid, rank, lo, transpose)
                rowptr, ci = shard_csr(rows, cols, hi - lo)
                halo, local, recv = halo_plan(ci, self.nid, self.cuts, rank)
                ranks.append(dict(rows=rows, cols=cols, rowptr=rowptr, colidx_orig=ci, halo=halo, colidx_local=local, recv_rows=recv,
                                  n_local=hi - lo))
            for rank, (want, counts, idx) in enumerate(send_lists([r["halo"] for r in ranks], self.cuts)):
                ranks[rank].update(want=want, send_rows=counts, send_idx=idx, slots=slot_table(idx, ranks[rank]["n_local"]))
            self.sides[transpose] = ranks
