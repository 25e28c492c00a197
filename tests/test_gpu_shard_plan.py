"""The 1-D vertex partition and the halo plan behind the C-ABI (gnn.cpp_amd/csrc/gnnx_shard.hip) held to their restatement (run with
-m gpu on an MI355X): gnnx_vertex_weights, gnnx_partition_deal, gnnx_partition_scramble, gnnx_shard_select_edges,
gnnx_halo_plan_create, gnnx_halo_plan_set_send_list, gnnx_halo_plan_info and gnnx_halo_plan_slot_table, call by call, on graphs
chosen for one edge each (tests/shard_ref.py `graph`: no vertices, no edges, only self loops, an unsorted list with duplicates, all
weights tied across a 256-thread block boundary, a hub that every peer reads, R-MAT, fewer vertices than ranks) at worlds 1, 2, 3, 8
and 9.

The reference is tests/shard_ref.py (NumPy and plain loops, written from include/gnnx.h; pinned to hand-written expectations and to
gnn.cpp_amd/shard.py by tests/test_shard_ref_cpu.py, which also shows that these cases tell a wrong tie break, a round-robin deal, a
missing scramble, a sorted selection and a wrong slot limit from the right ones).  Everything runs in one thread with no
communicator -- the test moves the halo lists between the ranks' plans itself -- and everything is integer work, so every comparison
is equality.  Every stage takes the RESTATED output of the stage before it as its input: a failure names the call that is wrong."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import shard_ref as R
from tests.helpers import synth

pytestmark = pytest.mark.gpu

INVALID_ARG, INDEX_RANGE = -1, -3      # include/gnnx.h
SENTINEL = -77
F = 8


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    sn = importlib.import_module("gnncpp_amd.shard_native")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, sn=sn, dev=torch.device("cuda:0"))


_PLANS = {}


def ref_plan(name, world, rw):
    """The restated plan of a combination, computed once and left unchanged."""
    key = (name, world, rw)
    if key not in _PLANS:
        src, dst, n = R.graph(name, synth)
        _PLANS[key] = R.Plan(src, dst, n, world, rw)
    return _PLANS[key]


def dev(env, a, dtype=np.int32):
    return env["torch"].from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1))).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64))


def plan_info(env, side):
    """(n_local, n_halo, n_send) straight from gnnx_halo_plan_info."""
    nl, nh, ns = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5)
    env["capi"].call("gnnx_halo_plan_info", side.h, C.byref(nl), C.byref(nh), C.byref(ns), None, None, None, None)
    return nl.value, nh.value, ns.value


def status_of(env, fn):
    """The status a refused call raises with."""
    with pytest.raises(env["capi"].GnnxError) as e:
        fn()
    return e.value.status


# ================================================================================================ partition
@pytest.mark.parametrize("name,world,rw", R.combinations())
def test_partition_equals_restatement(env, name, world, rw):
    sn = env["sn"]
    p = ref_plan(name, world, rw)
    src, dst, n = dev(env, p.src), dev(env, p.dst), p.n
    w = sn.vertex_weights(src, dst, n, rw)
    assert same(host(w), p.weight), "gnnx_vertex_weights"
    # the deal, from the restated weights
    owner, nid, cuts = sn.partition_deal(dev(env, p.weight), world)
    assert cuts == p.cuts, "gnnx_partition_deal: cuts"
    assert same(host(owner), p.owner), "gnnx_partition_deal: owner"
    assert same(host(nid), p.nid0), "gnnx_partition_deal: nid"
    # the scramble, from the restated deal
    nid2 = sn.partition_scramble(dev(env, p.owner), dev(env, p.nid0), p.cuts)
    assert same(host(nid2), p.nid), "gnnx_partition_scramble"
    # one rank needs no owner array
    if world == 1:
        assert same(host(sn.partition_scramble(None, dev(env, p.nid0), p.cuts)), p.nid)
    # properties that need no reference, on the native chain weights -> deal -> scramble
    o2, n2, c2 = sn.partition_deal(w, world)
    sn.partition_scramble(o2, n2, c2)
    o_h, n_h = host(o2), host(n2)
    assert c2[0] == 0 and c2[-1] == n and len(c2) == world + 1
    assert sorted(n_h.tolist()) == list(range(n)), "nid is not a permutation of [0, n)"
    for q in range(world):
        part = n_h[o_h == q]
        assert part.size == c2[q + 1] - c2[q] and (part.size == 0 or (part.min() >= c2[q] and part.max() < c2[q + 1]))
    counts = [c2[q + 1] - c2[q] for q in range(world)]
    assert max(counts) - min(counts) <= 1, "row counts per rank differ by more than 1"
    # a second run gives the same bits (integer atomics in the degree count)
    w_b = sn.vertex_weights(src, dst, n, rw)
    o_b, n_b, c_b = sn.partition_deal(w_b, world)
    sn.partition_scramble(o_b, n_b, c_b)
    assert same(host(w_b), host(w)) and same(host(o_b), o_h) and same(host(n_b), n_h) and c_b == c2


# ================================================================================================ selection
@pytest.mark.parametrize("name,world,rw", R.combinations())
def test_selection_equals_restatement(env, name, world, rw):
    torch, ops, capi = env["torch"], env["ops"], env["capi"]
    p = ref_plan(name, world, rw)
    src, dst, owner, nid = dev(env, p.src), dev(env, p.dst), dev(env, p.owner), dev(env, p.nid)
    E = int(p.src.size)
    for transpose in (False, True):
        for rank in range(world):
            r = p.sides[transpose][rank]
            rows = torch.full((max(E, 1),), SENTINEL, dtype=torch.int32, device=env["dev"])
            cols = torch.full((max(E, 1),), SENTINEL, dtype=torch.int32, device=env["dev"])
            nsel = C.c_int64(-5)
            capi.call("gnnx_shard_select_edges", ops._ptr(src), ops._ptr(dst), E, ops._ptr(owner), ops._ptr(nid), rank, p.cuts[rank],
                      int(transpose), ops._ptr(rows), ops._ptr(cols), C.byref(nsel), ops._stream())
            torch.cuda.synchronize()
            m = nsel.value
            what = f"rank {rank}, transpose {transpose}"
            assert m == r["rows"].size, what
            assert same(host(rows[:m]), r["rows"]) and same(host(cols[:m]), r["cols"]), what
            assert bool((rows[m:] == SENTINEL).all()) and bool((cols[m:] == SENTINEL).all()), what + ": wrote past n_selected"
    if name == "loops":
        assert all(r["rows"].size == 0 for t in (False, True) for r in p.sides[t])


# ================================================================================================ halo plan and send list
def _alternative_list(p, rank, n_local):
    """A second, different send list of rank `rank`: the next rank reads all its rows, last row first."""
    counts = [0] * p.world
    if p.world == 1 or n_local == 0:
        return np.zeros(0, dtype=np.int32), counts
    counts[(rank + 1) % p.world] = n_local
    return np.arange(p.cuts[rank + 1] - 1, p.cuts[rank] - 1, -1, dtype=np.int32), counts


@pytest.mark.parametrize("name,world,rw", R.combinations())
def test_halo_plan_and_send_list_equal_restatement(env, name, world, rw):
    torch, ops, capi, sn = env["torch"], env["ops"], env["capi"], env["sn"]
    p = ref_plan(name, world, rw)
    n = p.n
    src, dst, owner, nid = dev(env, p.src), dev(env, p.dst), dev(env, p.owner), dev(env, p.nid)
    ccuts = (C.c_int64 * (world + 1))(*p.cuts)
    for transpose in (False, True):
        sides = []
        for rank in range(world):
            r = p.sides[transpose][rank]
            what = f"rank {rank}, transpose {transpose}"
            # selection -> gnnx_csr_from_coo (max(n_local, n) rows, self loops kept) -> gnnx_halo_plan_create
            side = sn.NativeHaloSide(src, dst, owner, nid, p.cuts, rank, world, n, transpose)
            sides.append(side)
            assert same(host(side.rowptr), r["rowptr"]), what + ": rowptr of the shard"
            n_local, n_halo, n_send = plan_info(env, side)
            assert n_local == r["n_local"] == side.n_local and n_halo == r["halo"].size == side.n_halo, what
            assert side.recv_counts == r["recv_rows"], what
            assert same(host(side.halo(env["dev"])), r["halo"]), what + ": halo ids"
            assert same(host(side.colidx), r["colidx_local"]), what + ": colidx_local"
            if name == "loops":
                assert side.colidx.numel() == 0 and n_halo == 0
            # before any send list: none for several ranks, an empty one for one rank
            assert n_send == side.n_send == (0 if world == 1 else -1), what
            assert side.send_counts == ([0] if world == 1 else None) and side.slot_table(env["dev"]) is None, what
            # d_colidx_local may alias d_colidx_orig
            ci = dev(env, r["colidx_orig"])
            h = C.c_void_p()
            capi.call("gnnx_halo_plan_create", ops._ptr(ci), int(ci.numel()), ops._ptr(nid), n, world, rank, ccuts, ops._ptr(ci), C.byref(h),
                      ops._stream())
            torch.cuda.synchronize()
            nh = C.c_int64(-5)
            capi.call("gnnx_halo_plan_info", h, None, C.byref(nh), None, None, None, None, None)
            capi.call("gnnx_halo_plan_destroy", h)
            assert same(host(ci), r["colidx_local"]) and nh.value == r["halo"].size, what + ": aliased colidx"
        # the requests, moved by the test: owner `rank` gets from every peer q the part of q's halo list inside its range
        halos = [host(s.halo(env["dev"])) for s in sides]
        for rank, side in enumerate(sides):
            r = p.sides[transpose][rank]
            what = f"owner {rank}, transpose {transpose}"
            lo, hi = p.cuts[rank], p.cuts[rank + 1]
            parts = [h_[(h_ >= lo) & (h_ < hi)] for h_ in halos]
            counts = [int(x.size) for x in parts]
            want = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
            side.set_send_list(dev(env, want), counts)
            n_local, n_halo, n_send = plan_info(env, side)
            assert n_send == side.n_send == r["send_idx"].size and side.send_counts == r["send_rows"] == counts, what
            assert same(host(side.send_idx(env["dev"])), r["send_idx"]), what + ": send_idx"
            assert n_local == r["n_local"] and n_halo == r["halo"].size and side.recv_counts == r["recv_rows"], what
            table = side.slot_table(env["dev"])
            if n_send == 0 or r["slots"] is None:
                assert table is None, what + ": a slot table without a send list, or with a row of more than 7 slots"
            else:
                assert table is not None and same(host(table), r["slots"]), what + ": slot table"
            # a second list replaces the first, and its table
            want2, counts2 = _alternative_list(p, rank, r["n_local"])
            side.set_send_list(dev(env, want2) if want2.size else None, counts2)
            idx2 = want2 - lo
            assert plan_info(env, side)[2] == side.n_send == idx2.size and side.send_counts == counts2, what
            assert same(host(side.send_idx(env["dev"])), idx2), what + ": second send_idx"
            table = side.slot_table(env["dev"])
            if idx2.size == 0:
                assert table is None, what
            else:
                assert table is not None and same(host(table), R.slot_table(idx2, r["n_local"])), what + ": second slot table"
    if name == "star" and world in (8, 9):   # the hub's row: 7 slots keep the table, 8 drop it
        hub_rank = int(p.owner[R.STAR_HUB])
        assert (p.sides[False][hub_rank]["slots"] is None) == (world == 9)
        assert np.bincount(p.sides[False][hub_rank]["send_idx"]).max() == world - 1


# ================================================================================================ the plan means what it says
@pytest.mark.parametrize("world", [3, 8, 9])
@pytest.mark.parametrize("name", ["ring257", "star", "rmat"])
def test_plan_drives_the_single_gpu_aggregation(env, name, world):
    """Every rank's [local | halo] buffer, its tail filled from the owners' rows through their send lists (gnnx_gather_rows_f32),
    holds the rows the halo ids name, and the SpMM over the shard reproduces the single-GPU rows bit for bit, forward and backward."""
    torch, ops, sn = env["torch"], env["ops"], env["sn"]
    d = env["dev"]
    s_np, d_np, n = R.graph(name, synth)
    src, dst = dev(env, s_np), dev(env, d_np)
    g = ops.CsrGraph.from_coo(src, dst, n)
    H = ops.uniform_pm1(41, (n, F), device=d)
    G = ops.uniform_pm1(42, (n, F), device=d)
    out_ref = ops.aggregate_fwd(g, H, None, use_plan=False)
    dH_ref = ops.aggregate_bwd(g, G, use_plan=False)
    plans = [sn.NativeShardPlan(src, dst, n, rank, world, None, row_weight=3) for rank in range(world)]
    cuts = plans[0].cuts
    nid = plans[0].nid
    assert all(pl.cuts == cuts and torch.equal(pl.nid, nid) for pl in plans)
    orig = torch.empty(n, dtype=torch.int64, device=d)
    orig[nid.long()] = torch.arange(n, dtype=torch.int64, device=d)
    verts = [orig[cuts[q]:cuts[q + 1]] for q in range(world)]
    norm = g.norm.reshape(-1, 1)

    def fill(side_of, rank, rows):
        """[local | halo] rows of rank `rank`: local = rows[verts]; tail = for every owner q, q's local rows gathered with the segment
        of q's send list that is meant for `rank`."""
        side = side_of(plans[rank])
        parts = [rows[verts[rank]].contiguous()]
        for q in range(world):
            sq = side_of(plans[q])
            off, cnt = sum(sq.send_counts[:rank]), sq.send_counts[rank]
            assert cnt == side.recv_counts[q]
            if cnt:
                parts.append(ops.gather_rows(rows[verts[q]].contiguous(), sq.send_idx(d)[off:off + cnt].contiguous()))
        ext = torch.cat(parts).contiguous()
        assert ext.shape[0] == side.n_local + side.n_halo
        assert torch.equal(ext[side.n_local:], rows[orig[side.halo(d).long()]]), "the halo tail does not hold the rows its ids name"
        return ext

    for side_of in (lambda pl: pl.fwd, lambda pl: pl.bwd):
        halos = [host(side_of(pl).halo(d)) for pl in plans]
        for rank, pl in enumerate(plans):
            lo, hi = cuts[rank], cuts[rank + 1]
            parts = [h_[(h_ >= lo) & (h_ < hi)] for h_ in halos]
            side_of(pl).set_send_list(dev(env, np.concatenate(parts)), [int(x.size) for x in parts])
    for rank, pl in enumerate(plans):
        nl, v = pl.n_local, verts[rank]
        assert nl > 0
        Hext = fill(lambda x: x.fwd, rank, H)
        out = ops.spmm(pl.fwd.rowptr, pl.fwd.colidx, Hext, rowscale=g.norm[v].contiguous(), n_rows=nl)
        assert torch.equal(out, out_ref[v]), f"rank {rank}: forward aggregation over the shard is not bit-identical"
        Gext = fill(lambda x: x.bwd, rank, G)
        nb = fill(lambda x: x.bwd, rank, norm)
        dH = ops.spmm(pl.bwd.rowptr, pl.bwd.colidx, Gext, colscale=nb.reshape(-1).contiguous(), n_rows=nl)
        assert torch.equal(dH, dH_ref[v]), f"rank {rank}: backward aggregation over the shard is not bit-identical"


# ================================================================================================ refusals that need the device
def test_vertex_weights_refuses_an_endpoint_out_of_range(env):
    sn = env["sn"]
    s, d, n = R.graph("order")
    for bad_src, bad_dst in (([0, n], [1, 2]), ([0, 1], [n, 2]), ([0, -1], [1, 2])):
        st = status_of(env, lambda: sn.vertex_weights(dev(env, bad_src), dev(env, bad_dst), n, 1))
        assert st == INDEX_RANGE
    assert same(host(sn.vertex_weights(dev(env, s), dev(env, d), n, 3)), R.vertex_weights(s, d, n, 3))


def test_send_list_refusals(env):
    capi, sn = env["capi"], env["sn"]
    p = ref_plan("order", 2, 0)
    r = p.sides[False][0]
    side = sn.NativeHaloSide(dev(env, p.src), dev(env, p.dst), dev(env, p.owner), dev(env, p.nid), p.cuts, 0, 2, p.n, False)
    assert r["n_local"] == 3 and r["send_rows"] == [0, 2]

    def send_rows_status():
        sc = (C.c_int64 * 2)()
        return capi.lib().gnnx_halo_plan_info(side.h, None, None, None, None, sc, None, None)

    def no_list():
        return side.n_send == -1 and plan_info(env, side)[2] == -1 and send_rows_status() == INVALID_ARG and side.slot_table(env["dev"]) is None

    def holds_the_list():
        return (side.n_send == 2 and side.send_counts == r["send_rows"] and same(host(side.send_idx(env["dev"])), r["send_idx"])
                and same(host(side.slot_table(env["dev"])), r["slots"]))

    # send_rows before any send list
    assert no_list() and "not been set" in capi.lib().gnnx_last_error().decode()
    # a count for the rank itself, a negative count: refused, and still no list
    assert status_of(env, lambda: side.set_send_list(dev(env, [0, 1]), [1, 1])) == INVALID_ARG and no_list()
    assert status_of(env, lambda: side.set_send_list(dev(env, [0, 1]), [0, -2])) == INVALID_ARG and no_list()
    # a valid list works after them
    side.set_send_list(dev(env, r["want"]), r["send_rows"])
    assert holds_the_list()
    # the same refusals leave a list that is there alone
    assert status_of(env, lambda: side.set_send_list(dev(env, [0, 1]), [2, 0])) == INVALID_ARG and holds_the_list()
    assert status_of(env, lambda: side.set_send_list(dev(env, [0, 1]), [0, -1])) == INVALID_ARG and holds_the_list()
    # an id outside the rank's range [0, 3): the plan has no send list afterwards
    for bad in ([0, 3], [-1, 1]):
        assert status_of(env, lambda: side.set_send_list(dev(env, bad), [0, 2])) == INDEX_RANGE
        assert no_list()
        side.set_send_list(dev(env, r["want"]), r["send_rows"])
        assert holds_the_list()
