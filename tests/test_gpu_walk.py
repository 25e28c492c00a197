"""GPU tests of the random walks (run with -m gpu on an MI355X): gnnx_csr_random_walk through ops.random_walk / CsrGraph.random_walk,
ops.walk_pairs and EdgeSet.from_walks.  Integer work with one right answer: every device output is compared with tests/walk_ref.py
(Python integers, loops) by torch.equal.

Lane mapping (gnnx_walk.hip): a wavefront owns 64 consecutive walks and stages CHUNK = GNNX_WALK_CHUNK positions of them in LDS before
it stores them.  The seams are therefore the walks 64 * k and the positions CHUNK * k (position 0 is the start: a walk of L steps has
L + 1 positions)."""
import importlib
import os
import re

import numpy as np
import pytest

from tests import negative_ref as nr
from tests import sddmm_ref as sr
from tests import walk_ref as wr
from tests.helpers import ROOT, synth
from tests.test_walk_cpu import csr_of, golden_csr

pytestmark = pytest.mark.gpu

CHUNK = int(re.search(r"#define GNNX_WALK_CHUNK (\d+)", open(os.path.join(ROOT, "include", "gnnx.h")).read()).group(1))
SENTINEL = -77


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


def device_walks(env, csr, starts, L, seed, p=1.0, q=1.0, **kw):
    rowptr, colidx = csr
    return env["ops"].random_walk(dev(env, rowptr), dev(env, colidx), dev(env, np.asarray(starts, dtype=np.int32)), L, seed, p, q, **kw)


def assert_is_reference(env, csr, starts, L, seed, p=1.0, q=1.0, what=""):
    """The device walks equal the reference's, bit for bit; returns (reference walks, fallback steps, zero-weight steps)."""
    torch = env["torch"]
    ref, fb, zero = wr.walks_ref(csr[0], csr[1], starts, L, seed, p, q)
    got = device_walks(env, csr, starts, L, seed, p, q)
    assert got.dtype == torch.int32 and tuple(got.shape) == ref.shape, what
    assert torch.equal(got.cpu(), torch.from_numpy(ref)), f"{what}: the walks differ from the reference"
    return ref, fb, zero


@pytest.mark.parametrize("pq", [(1.0, 1.0), (0.5, 2.0)])
def test_lane_and_chunk_seams(env, pq):
    """Every (n_walks, L, ldw) cell against one reference: the key holds (walk number, step) alone, so fewer walks are the first rows
    and a shorter walk is a prefix.  ldw = L + 4: the pad behind each walk keeps its sentinel."""
    torch = env["torch"]
    csr = golden_csr("rmat64.npz")
    n = len(csr[0]) - 1
    n_max, L_max = 64 * 5 + 1, 2 * CHUNK + 1
    starts = np.array([(5 * x + 1) % n for x in range(n_max)], dtype=np.int32)
    ref = torch.from_numpy(wr.walks_ref(csr[0], csr[1], starts, L_max, 21, *pq)[0])
    rowptr, colidx, d_starts = dev(env, csr[0]), dev(env, csr[1]), dev(env, starts)
    for n_walks in (1, 63, 64, 65, n_max):
        for L in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, L_max):
            got = env["ops"].random_walk(rowptr, colidx, d_starts[:n_walks], L, 21, *pq)
            assert tuple(got.shape) == (n_walks, L + 1) and got.is_contiguous()
            assert torch.equal(got.cpu(), ref[:n_walks, :L + 1]), (n_walks, L)
            buf = torch.full((n_walks, L + 4), SENTINEL, dtype=torch.int32, device=env["dev"])
            view = env["ops"].random_walk(rowptr, colidx, d_starts[:n_walks], L, 21, *pq, out=buf)
            assert view.data_ptr() == buf.data_ptr() and tuple(view.shape) == (n_walks, L + 1)
            assert torch.equal(buf[:, :L + 1].cpu(), ref[:n_walks, :L + 1]), (n_walks, L, "padded")
            assert (buf[:, L + 1:] == SENTINEL).all(), (n_walks, L, "the pad was written")


@pytest.mark.parametrize("pq", [(1.0, 1.0), (0.5, 2.0)])
def test_dead_ends_and_bad_starts(env, pq):
    # directed: 0 -> 1 -> 2 and 4 <-> 5; 2 has no out-edge, 3 is isolated
    csr = csr_of([(0, 1), (1, 2), (4, 5), (5, 4)], 6, directed=True)
    starts = [4, 3, 5, 0, -1, 4, 6, 1, 5, 2, 4]
    ref, _, _ = assert_is_reference(env, csr, starts, 5, 3, *pq, what="dead ends")
    assert ref.tolist() == [[4, 5, 4, 5, 4, 5], [3, -1, -1, -1, -1, -1], [5, 4, 5, 4, 5, 4], [0, 1, 2, -1, -1, -1], [-1] * 6, [4, 5, 4, 5, 4, 5],
                            [-1] * 6, [1, 2, -1, -1, -1, -1], [5, 4, 5, 4, 5, 4], [2, -1, -1, -1, -1, -1], [4, 5, 4, 5, 4, 5]]
    got0 = device_walks(env, csr, starts, 0, 3, *pq)
    assert got0.cpu().tolist() == [[4], [3], [5], [0], [-1], [4], [-1], [1], [5], [2], [4]]
    # a CSR without entries (colidx may be null), and no walks at all
    empty = (np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert device_walks(env, empty, [0, 2, 3], 2, 1, *pq).cpu().tolist() == [[0, -1, -1], [2, -1, -1], [-1, -1, -1]]
    assert tuple(device_walks(env, csr, [], 4, 1, *pq).shape) == (0, 5)


def three_class_graph():
    """300 vertices, undirected: three hubs with 99 leaves each, a ring through the leaves and 300 uniform edges -- sparse, so that at
    p = 0.25, q = 4 most candidates of a hub weigh 1/16 and some steps exhaust their attempts."""
    n = 300
    edges = [(v, v % 3) for v in range(3, n)] + [(v, v + 1) for v in range(3, n - 1)]
    s, d = synth.uniform_edges(7, n, 300)
    edges += [(int(a), int(b)) for a, b in zip(s, d) if a != b]
    return csr_of(edges, n)


@pytest.fixture(scope="module")
def three(env):
    csr = three_class_graph()
    starts = [x % 3 if x % 4 else (37 * x) % 300 for x in range(1000)]      # three in four start at a hub
    return csr, starts


@pytest.mark.parametrize("pq", [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25), (0.25, 4.0)])
def test_all_three_classes(env, three, pq):
    csr, starts = three
    rowptr, colidx = csr
    L, seed = 10, 1
    ref, fb, zero = wr.walks_ref(rowptr, colidx, starts, L, seed, *pq)
    steps = int((ref[:, 1:] >= 0).sum())
    rows = [set(colidx[rowptr[v]:rowptr[v + 1]].tolist()) for v in range(len(rowptr) - 1)]
    seen = {wr.classify(int(ref[x, t + 1]), int(ref[x, t - 1]), rows[int(ref[x, t - 1])]) for x in range(len(starts)) for t in range(1, L)}
    print(f"{pq}: {steps} steps, {fb} through the fallback")
    assert seen == {0, 1, 2} and zero == 0
    if pq == (0.25, 4.0):       # before any device call: the seed was chosen so that the exact scan is exercised, and is not the rule
        assert 20 <= fb < steps // 2
    elif pq == (1.0, 1.0):
        assert fb == 0
    got = device_walks(env, csr, starts, L, seed, *pq)
    assert env["torch"].equal(got.cpu(), env["torch"].from_numpy(ref))


def test_forced_fallback_and_zero_weight(env):
    """A path 0 - 1 - 2: the step from a leaf has the single candidate u.  p = 2^20: threshold 2^12, the attempts fail, the exact scan
    takes it; p = 2^40: threshold 0, W == 0, the uniform fallback."""
    csr = csr_of([(0, 1), (1, 2)], 3)
    n, L = 70, 6
    for p, want_zero in ((2.0 ** 20, 0), (2.0 ** 40, 3 * n)):
        ref, fb, zero = assert_is_reference(env, csr, [1] * n, L, 17, p, 1.0, what=f"p = {p}")
        assert fb == 3 * n and zero == want_zero
        assert (ref[:, 0::2] == 1).all() and np.isin(ref[:, 1::2], (0, 2)).all()


@pytest.mark.parametrize("pq", [(2.0, 0.5), (1.0, 2.0 ** 20)])
def test_hub_row(env, pq):
    """A star with 5 000 leaves and a ring through them; walks go through the centre.  (2, 0.5): the membership search in the centre's
    row of 5 000 (a step from a leaf that came from the centre).  (1, 2^20), added here: at the centre all but three candidates weigh
    2^-20, so nearly every step there takes the scan over the 5 000 entries."""
    n = 5001
    csr = csr_of([(0, v) for v in range(1, n)] + [(v, v + 1) for v in range(1, n - 1)], n)
    starts = [0 if x % 2 else 1 + (97 * x) % (n - 1) for x in range(40)]
    ref, fb, zero = assert_is_reference(env, csr, starts, 6, 5, *pq, what=f"hub {pq}")
    assert (ref == 0).sum() >= 20 and zero == 0
    if pq[1] > 1:
        assert fb >= 20
    print(f"hub {pq}: {fb} steps through the fallback")


def test_repeats_and_slices(env):
    torch = env["torch"]
    csr = golden_csr("rmat64.npz")
    for pq in ((1.0, 1.0), (0.5, 2.0)):
        ref, _, _ = assert_is_reference(env, csr, [9] * 130, 20, 8, *pq, what="repeats")
        assert len({tuple(r) for r in ref.tolist()}) == 130          # the same start 130 times: pairwise different walks
        starts = [(11 * x) % 64 for x in range(130)]
        whole = device_walks(env, csr, starts, 20, 8, *pq)
        parts = [device_walks(env, csr, starts[a:b], 20, 8, *pq, walk_base=a) for a, b in ((0, 64), (64, 65), (65, 130))]
        assert torch.equal(torch.cat(parts), whole)
        assert not torch.equal(device_walks(env, csr, starts, 20, 8, *pq, walk_base=1), whole)
        assert not torch.equal(device_walks(env, csr, starts, 20, 9, *pq), whole)


def test_determinism(env, three):
    csr, starts = three
    for pq in ((1.0, 1.0), (0.25, 4.0)):
        assert env["torch"].equal(device_walks(env, csr, starts, 33, 4, *pq), device_walks(env, csr, starts, 33, 4, *pq))


def test_python_surface(env):
    """CsrGraph.random_walk, walk_pairs and EdgeSet.from_walks against the references."""
    torch, ops, capi = env["torch"], env["ops"], env["capi"]
    n = 64
    d = np.load(os.path.join(ROOT, "tests", "golden", "rmat64.npz"))
    src, dst = np.concatenate([d["src"], d["dst"]]), np.concatenate([d["dst"], d["src"]])
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n)
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    starts = np.array([3, 60, 3, 17, 41], dtype=np.int32)
    L, seed, pq = 5, 12, (0.5, 2.0)
    walks = g.random_walk(dev(env, starts), L, seed, *pq, walks_per_start=3)
    ref, _, _ = wr.walks_ref(rowptr, colidx, np.tile(starts, 3), L, seed, *pq)
    assert torch.equal(walks.cpu(), torch.from_numpy(ref))
    assert torch.equal(g.random_walk(dev(env, starts), L, seed).cpu(), torch.from_numpy(wr.walks_ref(rowptr, colidx, starts, L, seed)[0]))

    # a relabelled graph: rows are not ascending -- second-order walks are refused, uniform ones run
    gr = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n, relabel="scramble")
    with pytest.raises(capi.GnnxError, match="relabelled graph keeps each row in original-id order"):
        gr.random_walk(dev(env, starts), L, seed, *pq)
    with pytest.raises(capi.GnnxError):
        gr.random_walk(dev(env, starts), L, seed, q=2.0)
    got = gr.random_walk(dev(env, starts), L, seed, walks_per_start=2)
    assert torch.equal(got.cpu(), torch.from_numpy(wr.walks_ref(host(gr.rowptr), host(gr.colidx), np.tile(starts, 2), L, seed)[0]))

    # pairs
    window, m = 2, 2
    ps, pd = ops.walk_pairs(walks, window)
    rs, rd = wr.pairs_ref(ref, window)
    assert torch.equal(ps.cpu(), torch.from_numpy(rs)) and torch.equal(pd.cpu(), torch.from_numpy(rd))

    # EdgeSet.from_walks == from_pairs of the reference's distinct pairs (no (v, v)) with the reference negatives listed first
    e = ops.EdgeSet.from_walks(g, walks, window, m, seed)
    pos = sorted({(a, b) for a, b in zip(rs.tolist(), rd.tolist()) if a != b})
    pos_rows, pos_cols = np.array([a for a, _ in pos], dtype=np.int32), np.array([b for _, b in pos], dtype=np.int32)
    pos_rowptr = np.concatenate([[0], np.cumsum(np.bincount(pos_rows, minlength=n))]).astype(np.int32)
    neg, _ = nr.negatives_ref(pos_rowptr, rowptr, colidx, n, m, seed, 1)
    nsrc, ndst = np.repeat(pos_rows, m), neg.reshape(-1)
    keep = ndst >= 0
    label = np.concatenate([np.zeros(int(keep.sum())), np.ones(len(pos))]).astype(np.float32)
    want = ops.EdgeSet.from_pairs(dev(env, np.concatenate([nsrc[keep], pos_rows])), dev(env, np.concatenate([ndst[keep], pos_cols])),
                                  dev(env, label), n)
    for name in ("rowptr", "colidx", "target", "rowptr_t", "colidx_t", "map_t"):
        assert torch.equal(getattr(e, name), getattr(want, name)), name
    assert e.n == n and e.nnz == want.nnz > len(pos)
    pairs = list(zip(sr.row_of_entries(host(e.rowptr)).tolist(), host(e.colidx).tolist()))
    assert {pr for pr, t in zip(pairs, host(e.target)) if t == 1.0} == set(pos)
