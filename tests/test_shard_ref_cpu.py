"""CPU-side checks of the partition + halo plan restatement (tests/shard_ref.py) that tests/test_gpu_shard_plan.py holds
gnn.cpp_amd/csrc/gnnx_shard.hip to:
  * the restatement against expectations worked out by hand for graphs of up to 6 vertices, typed in as literals;
  * the restatement against gnn.cpp_amd/shard.py (deal_partition, scramble_nid, HaloSide) on CPU torch over the whole case list -- the
    reference the loopback tests already trust;
  * every case family can tell a wrong answer from a right one (the variants vary the restatement, never the project's code);
  * the argument refusals of the C-ABI that return before any device call."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import shard_ref as R
from tests.helpers import pkg, synth  # noqa: F401


def eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1))


# ------------------------------------------------------------------ by hand
def test_weights_by_hand():
    src, dst, n = R.graph("order")
    # out-degree 2 1 2 1 3 2, in-degree 3 2 2 2 1 1; the self loop (2, 2) counts twice for vertex 2, duplicates count as given
    assert eq(R.vertex_weights(src, dst, n, 0), [5, 3, 4, 3, 4, 3])
    assert eq(R.vertex_weights(src, dst, n, 3), [8, 6, 7, 6, 7, 6])
    assert eq(R.vertex_weights([], [], 4, 2), [2, 2, 2, 2])
    assert R.vertex_weights([], [], 0, 2).shape == (0,)
    s, d, _ = R.graph("loops")
    assert eq(R.vertex_weights(s, d, 5, 1), [3, 3, 1, 7, 3])
    with pytest.raises(ValueError):
        R.vertex_weights([0, 4], [1, 0], 4, 0)
    with pytest.raises(ValueError):
        R.vertex_weights([0], [-1], 4, 0)


def test_deal_by_hand():
    # order by (-w, id): 0 (5), 2 (4), 4 (4), 1 (3), 3 (3), 5 (3); snake over 2 ranks: 0 1 | 1 0 | 0 1
    owner, nid, cuts = R.deal([5, 3, 4, 3, 4, 3], 2)
    assert eq(owner, [0, 0, 1, 0, 1, 1]) and cuts == [0, 3, 6] and eq(nid, [0, 1, 3, 2, 4, 5])
    # all tied, 3 ranks, n = 5: 0 1 2 | 2 1
    owner, nid, cuts = R.deal([7, 7, 7, 7, 7], 3)
    assert eq(owner, [0, 1, 2, 2, 1]) and cuts == [0, 1, 3, 5] and eq(nid, [0, 1, 3, 4, 2])
    # n < world: ranks 3.. own nothing, the cuts repeat
    owner, nid, cuts = R.deal([1, 5, 5], 8)
    assert eq(owner, [2, 0, 1]) and cuts == [0, 1, 2, 3, 3, 3, 3, 3, 3] and eq(nid, [2, 0, 1])
    # one rank: the identity; no vertices: all-zero cuts
    owner, nid, cuts = R.deal([3, 1, 2], 1)
    assert eq(owner, [0, 0, 0]) and eq(nid, [0, 1, 2]) and cuts == [0, 3]
    owner, nid, cuts = R.deal([], 3)
    assert owner.shape == (0,) and nid.shape == (0,) and cuts == [0, 0, 0, 0]
    # three full rounds of a 2-rank snake: 0 1 | 1 0 | 0 1 on weights already in descending order
    owner, _, _ = R.deal([9, 8, 7, 6, 5, 4], 2)
    assert eq(owner, [0, 1, 1, 0, 0, 1])


def test_scramble_by_hand():
    # 2654435761 = 7 * 379205108 + 5: position k of 7 rows moves to 5 k mod 7
    assert R.SCRAMBLE_MUL == 2654435761 and R.SCRAMBLE_MUL % 7 == 5
    assert eq(R.scramble([0] * 7, list(range(7)), [0, 7]), [0, 5, 3, 1, 6, 4, 2])
    # two ranks: 7 rows from new id 2 on (rank 1), 2 rows before them (rank 0; the multiplier is odd: 2 rows stay)
    owner = [1, 0, 1, 1, 1, 0, 1, 1, 1]
    nid = [2, 0, 3, 4, 5, 1, 6, 7, 8]
    assert eq(R.scramble(owner, nid, [0, 2, 9]), [2, 0, 7, 5, 3, 1, 8, 6, 4])
    # 2654435761 mod 3, 4, 5, 6 = 1: ranges of up to 6 rows stay as they are (test_scramble_is_not_the_identity_... finds the others)
    for n_p in (1, 2, 3, 4, 5, 6):
        assert eq(R.scramble([0] * n_p, list(range(n_p)), [0, n_p]), list(range(n_p)))


def test_selection_by_hand():
    src, dst, n = R.graph("order")
    owner, nid = [0, 0, 1, 0, 1, 1], [0, 1, 3, 2, 4, 5]
    # edges (4,1) (0,3) (5,0) (2,2) (4,1) (1,5) (3,4) (0,3) (5,2) (2,0) (4,0)
    rows, cols = R.select_edges(src, dst, owner, nid, 0, 0, False)
    assert eq(rows, [0, 1, 2, 0]) and eq(cols, [3, 5, 4, 3])
    rows, cols = R.select_edges(src, dst, owner, nid, 1, 3, False)
    assert eq(rows, [1, 2, 1, 2, 0, 1]) and eq(cols, [1, 0, 1, 2, 0, 0])
    rows, cols = R.select_edges(src, dst, owner, nid, 0, 0, True)
    assert eq(rows, [1, 2, 0, 1, 2, 0, 0]) and eq(cols, [4, 0, 5, 4, 0, 2, 4])
    rows, cols = R.select_edges(src, dst, owner, nid, 1, 3, True)
    assert eq(rows, [2, 1, 0]) and eq(cols, [1, 3, 5])
    s, d, _ = R.graph("loops")
    rows, cols = R.select_edges(s, d, [0] * 5, list(range(5)), 0, 0, False)
    assert rows.shape == (0,) and cols.shape == (0,)


def test_halo_plan_and_send_lists_by_hand():
    nid, cuts = [0, 1, 3, 2, 4, 5], [0, 3, 6]
    # rank 0 forward: rows (0,3) (1,5) (2,4) after the build; columns 5 and 4 are remote (new ids 5 and 4)
    rowptr, ci = R.shard_csr([0, 1, 2, 0], [3, 5, 4, 3], 3)
    assert eq(rowptr, [0, 1, 2, 3]) and eq(ci, [3, 5, 4])
    halo0, local, recv = R.halo_plan(ci, nid, cuts, 0)
    assert eq(halo0, [4, 5]) and eq(local, [2, 4, 3]) and recv == [0, 2]
    # rank 1 forward: (0,0) (1,0) (1,1) (2,0) (2,2); column 2 is local row 0, columns 0 and 1 are remote
    rowptr, ci = R.shard_csr([1, 2, 1, 2, 0, 1], [1, 0, 1, 2, 0, 0], 3)
    assert eq(rowptr, [0, 1, 3, 5]) and eq(ci, [0, 0, 1, 0, 2])
    halo1, local, recv = R.halo_plan(ci, nid, cuts, 1)
    assert eq(halo1, [0, 1]) and eq(local, [3, 3, 4, 3, 0]) and recv == [2, 0]
    (want0, rows0, idx0), (want1, rows1, idx1) = R.send_lists([halo0, halo1], cuts)
    assert eq(want0, [0, 1]) and rows0 == [0, 2] and eq(idx0, [0, 1])
    assert eq(want1, [4, 5]) and rows1 == [2, 0] and eq(idx1, [1, 2])
    # three ranks, cuts 0 2 4 6: rank 1 is asked by rank 0 for 2, 3 and by rank 2 for 3: peer-major, row 1 twice
    out = R.send_lists([[2, 3, 5], [0, 4], [1, 3]], [0, 2, 4, 6])
    assert eq(out[0][0], [0, 1]) and out[0][1] == [0, 1, 1] and eq(out[0][2], [0, 1])
    assert eq(out[1][0], [2, 3, 3]) and out[1][1] == [2, 0, 1] and eq(out[1][2], [0, 1, 1])
    assert eq(out[2][0], [5, 4]) and out[2][1] == [1, 1, 0] and eq(out[2][2], [1, 0])
    # no columns at all
    halo, local, recv = R.halo_plan([], nid, cuts, 1)
    assert halo.shape == (0,) and local.shape == (0,) and recv == [0, 0]


def test_slot_table_by_hand():
    t = R.slot_table([2, 0, 2, 2], 3)
    m = -1
    assert t.dtype == np.int32 and t.tolist() == [[1, m, m, m, m, m, m, m], [m] * 8, [0, 2, 3, m, m, m, m, m]]
    assert R.slot_table([1] * 7, 2).tolist() == [[m] * 8, [0, 1, 2, 3, 4, 5, 6, m]]
    assert R.slot_table([1] * 8, 2) is None
    assert R.slot_table([0, 1] * 7 + [1], 2) is None
    assert R.slot_table([], 2).tolist() == [[m] * 8, [m] * 8]


# ------------------------------------------------------------------ against shard.py on CPU torch
@pytest.fixture(scope="module")
def plans():
    """The restated plan of every combination, built once and left unchanged."""
    out = {}
    for name, world, rw in R.combinations():
        src, dst, n = R.graph(name, synth)
        out[name, world, rw] = R.Plan(src, dst, n, world, rw)
    return out


def test_case_list_is_the_one_the_gpu_tests_run():
    combos = R.combinations()
    assert len(set(combos)) == len(combos) == 7 * 10 + 2 + 4
    by_name = {}
    for name, world, rw in combos:
        by_name.setdefault(name, set()).add((world, rw))
    full = {(w, rw) for w in (1, 2, 3, 8, 9) for rw in (0, 3)}
    for name in ("lonely1", "lonely5", "loops", "order", "ring257", "star", "rmat"):
        assert by_name[name] == full
    assert by_name["few"] == {(8, 0), (8, 3)} and by_name["empty"] == {(1, 0), (1, 3), (3, 0), (3, 3)}
    assert [R.graph(k, synth)[2] for k in ("empty", "lonely1", "lonely5", "loops", "order", "ring257", "star", "rmat", "few")] == \
        [0, 1, 5, 5, 6, 257, 40, 1000, 3]
    s, d, n = R.graph("rmat", synth)
    assert s.size == 8000 and len(set(zip(s.tolist(), d.tolist()))) < 8000 and bool((s == d).any())   # duplicates and self loops
    assert (np.bincount(s, minlength=n) == 0).any()                                                     # empty rows


@pytest.mark.parametrize("name,world,rw", R.combinations())
def test_restatement_equals_shard_py(plans, name, world, rw):
    import torch
    shard = importlib.import_module("gnncpp_amd.shard")
    p = plans[name, world, rw]
    n = p.n
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64).reshape(-1))   # noqa: E731
    w = torch.bincount(t64(p.src), minlength=n) + torch.bincount(t64(p.dst), minlength=n) + rw   # ShardPlan's cost model
    assert eq(p.weight, w.numpy())
    owner, nid0, cuts = shard.deal_partition(w, world, scramble=False)
    assert eq(p.owner, owner.numpy()) and eq(p.nid0, nid0.numpy()) and p.cuts == [int(c) for c in cuts]
    if n:
        assert eq(p.nid, shard.scramble_nid(owner, nid0, cuts).numpy())
    assert eq(p.nid, shard.deal_partition(w, world)[1].numpy())
    nid_t = t64(p.nid)
    for transpose in (False, True):
        sides = []
        for rank, r in enumerate(p.sides[transpose]):
            lo, hi = p.cuts[rank], p.cuts[rank + 1]
            # ShardPlan's selection: torch masks on the edge list
            s_, d_ = t64(p.src), t64(p.dst)
            a, b = (d_, s_) if transpose else (s_, d_)
            mine = (s_ != d_) & (t64(p.owner)[a] == rank) if n else torch.zeros(0, dtype=torch.bool)
            assert eq(r["rows"], (nid_t[a[mine]] - lo).numpy()) and eq(r["cols"], b[mine].numpy())
            side = shard.HaloSide(torch.from_numpy(r["rowptr"]), nid_t[t64(r["colidx_orig"])].to(torch.int32), lo, hi, p.cuts)
            assert side.n_local == r["n_local"] and side.n_halo == r["halo"].size
            assert eq(r["halo"], side.halo.numpy()) and eq(r["colidx_local"], side.colidx.numpy())
            assert r["recv_rows"] == side.recv_counts
            sides.append(side)
        # the requests, moved by hand: owner `rank` gets from every peer q the part of q's halo in its range
        for rank, r in enumerate(p.sides[transpose]):
            lo, hi = p.cuts[rank], p.cuts[rank + 1]
            parts = [s.halo[(s.halo >= lo) & (s.halo < hi)] for s in sides]
            assert r["send_rows"] == [int(x.numel()) for x in parts] == [s.recv_counts[rank] for s in sides]
            want = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int32)
            assert eq(r["want"], want.numpy())
            sides[rank].set_send_lists((want - lo).to(torch.int32), r["send_rows"])
            assert eq(r["send_idx"], sides[rank].send_idx.numpy())
            ops = importlib.import_module("gnncpp_amd.ops")
            table = ops.slot_table(sides[rank].send_idx, r["n_local"])
            if r["slots"] is None:
                assert table is None
            elif r["n_local"]:
                assert np.array_equal(r["slots"], table.numpy())


# ------------------------------------------------------------------ the cases can tell wrong from right
def test_tied_weights_tell_the_tie_break(plans):
    """ring257: every weight is equal, so the order is the tie break alone -- a descending-id tie break gives another owner."""
    for world in (2, 3, 8, 9):
        p = plans["ring257", world, 0]
        assert len(set(p.weight.tolist())) == 1
        w = p.weight.tolist()
        descending = sorted(range(p.n), key=lambda v: (-w[v], -v))
        assert not eq(p.owner, R.deal_from(descending, R.snake_rank, world)[0])
    p = plans["rmat", 8, 3]   # many ties next to distinct weights
    w = p.weight.tolist()
    assert 1 < len(set(w)) < p.n // 4
    assert not eq(p.owner, R.deal_from(sorted(range(p.n), key=lambda v: (-w[v], -v)), R.snake_rank, 8)[0])


def test_snake_deal_differs_from_round_robin(plans):
    for (name, world, rw), p in plans.items():
        round_robin = R.deal_from(R.deal_order(p.weight), lambda k, P: k % P, world)[0]
        assert eq(p.owner, round_robin) == (world == 1 or p.n <= world), (name, world)   # the second round is the first to differ
        if p.n >= 2 * world and world > 1:
            assert not eq(p.owner, round_robin)
    assert any(p.n >= 2 * w and w > 1 for (_, w, _), p in plans.items())


def test_scramble_is_not_the_identity_where_the_multiplier_is_not_one(plans):
    """Position 1 of n_p rows moves to 2654435761 mod n_p: the scramble is the identity exactly when that is 1 (n_p = 3, 4, 5, 6, 8,
    10, 16, ...) for every rank with at least 2 rows.  ring257 and rmat have ranks where it is not at every world, star at world 3."""
    moved = set()
    for (name, world, rw), p in plans.items():
        counts = [p.cuts[q + 1] - p.cuts[q] for q in range(world)]
        moves = any(c >= 2 and R.SCRAMBLE_MUL % c != 1 for c in counts)
        assert eq(p.nid, p.nid0) == (not moves), (name, world)
        if moves:
            moved.add((name, world))
        assert sorted(p.nid.tolist()) == list(range(p.n))
    for name in ("ring257", "rmat"):
        assert all((name, w) in moved for w in R.WORLDS)
    assert ("star", 3) in moved and ("star", 8) not in moved       # ranks of 14 and 13 rows; of 5 rows


def test_edge_order_case_is_not_sorted(plans):
    """A selection that sorted its output (by row or by column) or dropped duplicates would differ from the one in edge order: at
    every world and in both transpositions some rank's selection is in neither order, and some rank's holds a pair twice."""
    for world in R.WORLDS:
        p = plans["order", world, 0]
        for transpose in (False, True):
            unsorted = repeated = 0
            for r in p.sides[transpose]:
                pairs = list(zip(r["rows"].tolist(), r["cols"].tolist()))
                unsorted += pairs != sorted(pairs) and pairs != sorted(pairs, key=lambda x: (x[1], x[0]))
                repeated += len(set(pairs)) < len(pairs)
            assert unsorted >= 1 and repeated >= 1, (world, transpose)
    src, dst, _ = R.graph("order")
    keys = [(s, d) for s, d in zip(src.tolist(), dst.tolist())]
    assert keys != sorted(keys) and (2, 2) in keys and len(set(keys)) < len(keys)


def test_star_hub_row_has_seven_slots_at_world_8_and_eight_at_world_9(plans):
    for rw in R.ROW_WEIGHTS:
        for transpose in (False, True):
            for world, slots in ((8, 7), (9, 8)):
                p = plans["star", world, rw]
                rank = int(p.owner[R.STAR_HUB])
                r = p.sides[transpose][rank]
                hub_row = int(p.nid[R.STAR_HUB]) - p.cuts[rank]
                assert r["send_idx"].tolist().count(hub_row) == slots == world - 1
                assert max(np.bincount(r["send_idx"], minlength=r["n_local"])) == slots
                if slots == 7:
                    assert r["slots"] is not None and r["slots"][hub_row].tolist() == sorted(r["slots"][hub_row, :7].tolist()) + [-1]
                    assert int((r["slots"][hub_row] >= 0).sum()) == 7
                else:
                    assert r["slots"] is None
                # every other rank's rows are read by the hub's owner alone: their tables exist at both worlds
                assert all(q["slots"] is not None for k, q in enumerate(p.sides[transpose]) if k != rank)


def test_few_case_has_ranks_without_rows(plans):
    p = plans["few", 8, 0]
    assert p.cuts[3:] == [3] * 6 and [r["n_local"] for r in p.sides[False]] == [1, 1, 1, 0, 0, 0, 0, 0]
    assert all(r["halo"].size == 0 and r["send_idx"].size == 0 for r in p.sides[False][3:])
    assert all(r["halo"].size > 0 for r in p.sides[False][:3])


# ------------------------------------------------------------------ refusals before any device call
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


SHARD_SYMBOLS = ["gnnx_vertex_weights", "gnnx_partition_deal", "gnnx_partition_scramble", "gnnx_shard_select_edges", "gnnx_halo_plan_create",
                 "gnnx_halo_plan_destroy", "gnnx_halo_plan_info", "gnnx_halo_plan_set_send_list", "gnnx_halo_plan_exchange_requests",
                 "gnnx_halo_plan_slot_table"]
OK, INVALID, INDEX_RANGE, UNSUPPORTED = 0, -1, -3, -7


def test_shard_entry_points_are_declared_exported_and_bound(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for name in SHARD_SYMBOLS:
        assert name in declared and hasattr(L, name) and name in capi._SIGS
    sn = importlib.import_module("gnncpp_amd.shard_native")
    for name in ("vertex_weights", "partition_deal", "partition_scramble"):
        assert callable(getattr(sn, name))
    assert callable(sn.NativeHaloSide.set_send_list)


def test_shard_argument_refusals_without_device(capi):
    """What the partition and plan calls refuse before they touch a device.  The pointers that stand for device arrays are never
    followed on these paths: any non-null value will do."""
    L = capi.lib()
    dev = C.c_void_p(0x1000)
    err = lambda: L.gnnx_last_error().decode()   # noqa: E731
    # gnnx_vertex_weights: negative sizes; no vertices is an early OK
    assert L.gnnx_vertex_weights(dev, dev, -1, 4, 0, dev, None) == INVALID and "negative" in err()
    assert L.gnnx_vertex_weights(dev, dev, 4, -1, 0, dev, None) == INVALID
    assert L.gnnx_vertex_weights(dev, dev, 4, 4, -1, dev, None) == INVALID
    assert L.gnnx_vertex_weights(None, None, 0, 0, 3, None, None) == OK
    # gnnx_partition_deal
    cuts = (C.c_int64 * 10)(*([-7] * 10))
    assert L.gnnx_partition_deal(dev, -1, 2, dev, dev, cuts, None) == INVALID
    assert L.gnnx_partition_deal(dev, 4, 0, dev, dev, cuts, None) == INVALID
    assert L.gnnx_partition_deal(dev, 4, -3, dev, dev, cuts, None) == INVALID
    assert L.gnnx_partition_deal(dev, 4, 2, dev, dev, None, None) == INVALID
    assert list(cuts) == [-7] * 10                                             # a refused call writes nothing
    assert L.gnnx_partition_deal(dev, 1 << 30, 2, dev, dev, cuts, None) == UNSUPPORTED and "2^31" in err()
    assert L.gnnx_partition_deal(dev, (1 << 31) - 1, 1, dev, dev, None, None) == INVALID
    assert L.gnnx_partition_deal(None, 0, 3, None, None, cuts, None) == OK and list(cuts) == [0, 0, 0, 0] + [-7] * 6
    # gnnx_partition_scramble
    c2 = (C.c_int64 * 3)(0, 2, 4)
    assert L.gnnx_partition_scramble(dev, -1, 2, c2, dev, None) == INVALID
    assert L.gnnx_partition_scramble(dev, 4, 0, c2, dev, None) == INVALID
    assert L.gnnx_partition_scramble(dev, 4, 2, None, dev, None) == INVALID
    assert L.gnnx_partition_scramble(dev, 4, 2, c2, None, None) == INVALID
    assert L.gnnx_partition_scramble(None, 4, 2, c2, dev, None) == INVALID and "owner" in err()
    assert L.gnnx_partition_scramble(dev, 5, 2, c2, dev, None) == INVALID and "partition" in err()          # cuts[world] != n
    assert L.gnnx_partition_scramble(dev, 4, 2, (C.c_int64 * 3)(1, 2, 4), dev, None) == INVALID             # cuts[0] != 0
    assert L.gnnx_partition_scramble(dev, 4, 2, (C.c_int64 * 3)(0, 5, 4), dev, None) == INVALID             # not monotone
    assert L.gnnx_partition_scramble(None, 0, 2, (C.c_int64 * 3)(0, 0, 0), None, None) == OK
    # gnnx_shard_select_edges
    nsel = C.c_int64(-7)
    assert L.gnnx_shard_select_edges(dev, dev, -1, dev, dev, 0, 0, 0, dev, dev, C.byref(nsel), None) == INVALID
    assert L.gnnx_shard_select_edges(dev, dev, 4, dev, dev, -1, 0, 0, dev, dev, C.byref(nsel), None) == INVALID
    assert L.gnnx_shard_select_edges(dev, dev, 4, dev, dev, 0, 0, 0, dev, dev, None, None) == INVALID
    assert L.gnnx_shard_select_edges(dev, dev, 1 << 31, dev, dev, 0, 0, 0, dev, dev, C.byref(nsel), None) == UNSUPPORTED and "2^31" in err()
    assert nsel.value == -7
    assert L.gnnx_shard_select_edges(None, None, 0, None, None, 0, 0, 1, None, None, C.byref(nsel), None) == OK and nsel.value == 0
    nsel = C.c_int64(-7)
    assert L.gnnx_shard_select_edges(None, dev, 4, dev, dev, 0, 0, 0, dev, dev, C.byref(nsel), None) == INVALID and nsel.value == 0
    # gnnx_halo_plan_create
    plan = C.c_void_p(0)
    good = (C.c_int64 * 4)(0, 2, 4, 6)
    create = lambda nnz, n, world, rank, cuts_, out=C.byref(plan): L.gnnx_halo_plan_create(dev, nnz, dev, n, world, rank, cuts_, dev, out, None)   # noqa: E731
    assert create(3, 6, 3, 3, good) == INVALID                                  # rank >= world
    assert create(3, 6, 3, -1, good) == INVALID
    assert create(3, 6, 0, 0, good) == INVALID                                  # world < 1
    assert create(-1, 6, 3, 0, good) == INVALID
    assert create(3, -1, 3, 0, good) == INVALID
    assert create(3, 6, 3, 0, None) == INVALID
    assert create(3, 6, 3, 0, good, None) == INVALID                            # no place for the plan
    assert create(3, 6, 3, 0, (C.c_int64 * 4)(1, 2, 4, 6)) == INVALID and "0 to n_nodes" in err()
    assert create(3, 7, 3, 0, good) == INVALID and "0 to n_nodes" in err()      # cuts[world] != n_nodes
    assert create(3, 6, 3, 0, (C.c_int64 * 4)(0, 4, 2, 6)) == INVALID and "monotone" in err()
    assert L.gnnx_halo_plan_create(None, 3, dev, 6, 3, 0, good, dev, C.byref(plan), None) == INVALID and "null" in err()
    assert L.gnnx_halo_plan_create(dev, 3, None, 6, 3, 0, good, dev, C.byref(plan), None) == INVALID
    assert L.gnnx_halo_plan_create(dev, 3, dev, 6, 3, 0, good, None, C.byref(plan), None) == INVALID
    assert not plan.value                                                        # no refused call made a plan
    # a null plan, null out pointers
    i64 = C.c_int64(0)
    assert L.gnnx_halo_plan_info(None, C.byref(i64), None, None, None, None, None, None) == INVALID and "plan is null" in err()
    assert L.gnnx_halo_plan_set_send_list(None, dev, (C.c_int64 * 2)(0, 0), None) == INVALID
    assert L.gnnx_halo_plan_exchange_requests(None, None, None) == INVALID
    p = C.c_void_p(0x55)
    assert L.gnnx_halo_plan_slot_table(None, C.byref(p)) == INVALID and p.value == 0x55
    assert L.gnnx_halo_plan_destroy(None) == OK
