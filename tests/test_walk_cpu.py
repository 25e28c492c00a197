"""CPU tests of the random walks (no GPU needed): the reference restatement tests/walk_ref.py against hand-written literals, its own
invariants and the enumerated node2vec distribution; ops.walk_pairs (plain torch slicing) on a literal; the header, the exports and the
argument validation of gnnx_csr_random_walk, which happens before any device call."""
import ctypes as C
import importlib
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import walk_ref as wr
from tests.helpers import ROOT, synth

# h(w, t, a) of the contract at two seeds, from an independent evaluation of the key with synth.splitmix64 (uint64 wrap-around)
KEYS = {
    (2024, 0, 0, 0): 0x2E2FDCFF0B9C1EE6, (2024, 1, 0, 0): 0xE836644CB0E7B46D, (2024, 0, 1, 0): 0x298799907385D5B6,
    (2024, 0, 1, 1): 0x4320D577796E8248, (2024, 5, 3, 128): 0x2A6511289EDE5CF1, (2024, 2 ** 32 - 1, 79, 127): 0xCC3FD09E354A2A4F,
    (0xDEADBEEFCAFEF00D, 0, 0, 0): 0xBA96D4CF5FE750CE, (0xDEADBEEFCAFEF00D, 1, 0, 0): 0x0EAEF0CAC07B04FB,
    (0xDEADBEEFCAFEF00D, 0, 1, 0): 0x738704DCF9160A05, (0xDEADBEEFCAFEF00D, 0, 1, 1): 0xB790957802E4D722,
    (0xDEADBEEFCAFEF00D, 5, 3, 128): 0xE971E4E5A7FA0D5C, (0xDEADBEEFCAFEF00D, 2 ** 32 - 1, 79, 127): 0xAEB306F6C2B73D7B,
}
# (thr_a, thr_b, thr_c) by hand: weights (1/p, 1, 1/q) over their maximum, times 2^32
THRESHOLDS = {
    (1.0, 1.0): (2 ** 32, 2 ** 32, 2 ** 32),
    (0.25, 4.0): (2 ** 32, 2 ** 30, 2 ** 28),         # (4, 1, 1/4) / 4
    (2.0 ** 20, 1.0): (2 ** 12, 2 ** 32, 2 ** 32),    # (2^-20, 1, 1)
}

# 6 vertices, undirected.  At (u, v) = (0, 1) row 1 = [0, 2, 3, 4, 5] holds all three classes: 0 is u; 2 and 4 are neighbours of 0;
# 3 and 5 are not.  Row 0 = [1, 2, 4].
SIX_EDGES = [(0, 1), (0, 2), (0, 4), (1, 2), (1, 3), (1, 4), (1, 5)]


def csr_of(edges, n, directed=False):
    rows = [set() for _ in range(n)]
    for a, b in edges:
        rows[a].add(b)
        if not directed:
            rows[b].add(a)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.array([c for r in rows for c in sorted(r)], dtype=np.int32)
    return rowptr, colidx


def golden_csr(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name))
    return csr_of(zip(d["src"].tolist(), d["dst"].tolist()), int(d["X"].shape[0]))   # both directions: an undirected graph


def test_key_and_thresholds_are_the_header_formulas():
    G = np.uint64(wr.GOLDEN)

    def sm(x):
        return synth.splitmix64(np.array([x], dtype=np.uint64))[0]

    for (seed, w, t, a), want in KEYS.items():
        assert wr.h(seed, w, t, a) == want, (seed, w, t, a)
        with np.errstate(over="ignore"):
            s = sm(np.uint64(seed) ^ np.uint64(0x77616C6B73746570))
            assert int(sm(sm(s ^ (np.uint64((w << 32) | t) * G)) ^ (np.uint64(a) * G))) == want
    assert wr.DOMAIN == int.from_bytes(b"walkstep", "big")
    assert wr.h(1, 3, 4, 0) != wr.h(1 + 2 ** 32, 3, 4, 0)        # all 64 bits of the seed count
    from tests import negative_ref as nr
    assert wr.h(7, 1, 2, 3) != nr.key(7, 1, 2, 3)                # the domain constant separates the draw from the negative sampler's
    for pq, want in THRESHOLDS.items():
        assert wr.thresholds(*pq) == want, pq
    assert wr.thresholds(2.0 ** 40, 1.0)[0] == 0                 # below the 2^-32 quantum: a class that is never accepted
    assert wr.thresholds(4.0, 0.25) == (2 ** 28, 2 ** 30, 2 ** 32)


@pytest.mark.parametrize("pq", [(1.0, 1.0), (0.5, 2.0), (0.25, 4.0), (4.0, 0.25)])
def test_steps_follow_stored_entries_and_slices_equal_the_whole(pq):
    rowptr, colidx = golden_csr("rmat64.npz")
    n = len(rowptr) - 1
    starts = [(7 * x) % n for x in range(40)]
    L = 9
    walks, _, _ = wr.walks_ref(rowptr, colidx, starts, L, 11, *pq)
    assert walks.shape == (40, L + 1) and np.array_equal(walks[:, 0], starts)
    for x in range(40):
        for t in range(L):
            v, nxt = int(walks[x, t]), int(walks[x, t + 1])
            if v < 0 or rowptr[v + 1] == rowptr[v]:
                assert (walks[x, t + 1:] == -1).all()            # -1 is absorbing, a vertex without neighbours ends the walk
                break
            assert nxt in colidx[rowptr[v]:rowptr[v + 1]]
    parts = [wr.walks_ref(rowptr, colidx, starts[a:b], L, 11, *pq, walk_base=a)[0] for a, b in ((0, 13), (13, 14), (14, 40))]
    assert np.array_equal(np.concatenate(parts), walks)
    # the key holds the walk number, not the start: another base gives other walks from the same starts
    assert not np.array_equal(wr.walks_ref(rowptr, colidx, starts, L, 11, *pq, walk_base=1)[0], walks)


def test_dead_ends_and_bad_starts():
    # directed: 0 -> 1 -> 2, 2 has no out-edge; 3 is isolated
    rowptr, colidx = csr_of([(0, 1), (1, 2)], 4, directed=True)
    walks, fb, zero = wr.walks_ref(rowptr, colidx, [0, 3, -1, 4, 2, 1], 4, 5, 0.5, 2.0)
    assert walks.tolist() == [[0, 1, 2, -1, -1], [3, -1, -1, -1, -1], [-1] * 5, [-1] * 5, [2, -1, -1, -1, -1], [1, 2, -1, -1, -1]]
    assert (fb, zero) == (0, 0)
    assert wr.walks_ref(rowptr, colidx, [0, 3, -1, 4], 0, 5)[0].tolist() == [[0], [3], [-1], [-1]]


def test_general_path_at_p_q_1_has_the_uniform_bits():
    rowptr, colidx = golden_csr("rmat64.npz")
    starts = list(range(len(rowptr) - 1))
    uni, fb, _ = wr.walks_ref(rowptr, colidx, starts, 12, 3)
    gen, fb_g, _ = wr.walks_ref(rowptr, colidx, starts, 12, 3, general=True)
    assert np.array_equal(uni, gen) and fb == fb_g == 0
    # and the uniform step is the formula itself
    for x in (0, 5, 63):
        v = starts[x]
        d = int(rowptr[v + 1] - rowptr[v])
        if d:
            assert uni[x, 1] == colidx[rowptr[v] + ((wr.h(3, x, 0, 0) * d) >> 64)]


def _within_5_sd(counts, probs, n):
    for k, (c, pr) in enumerate(zip(counts, probs)):
        pr = float(pr)
        sd = math.sqrt(n * pr * (1 - pr))
        assert abs(c - n * pr) <= 5 * sd + 1e-9, (k, c, n * pr, sd)


@pytest.mark.parametrize("pq,tries", [((0.25, 4.0), wr.TRIES), ((2.0, 0.5), wr.TRIES), ((0.25, 4.0), 0), ((2.0 ** 20, 0.5), 0)])
def test_step_distribution_against_enumeration(pq, tries):
    """40 000 reference steps from v = 1 that came from u = 0 on the 6-vertex graph, against the enumerated probabilities, per entry and
    per class.  tries = 0 forces every step through the exact fallback."""
    rowptr, colidx = csr_of(SIX_EDGES, 6)
    row_v, row_u = colidx[rowptr[1]:rowptr[2]].tolist(), colidx[rowptr[0]:rowptr[1]].tolist()
    assert row_v == [0, 2, 3, 4, 5] and row_u == [1, 2, 4]
    assert sorted({wr.classify(x, 0, set(row_u)) for x in row_v}) == [0, 1, 2]
    thr = wr.thresholds(*pq)
    probs = wr.node2vec_probs(row_v, 0, row_u, *pq)
    wts = [1 / pq[0], 1.0, 1 / pq[1], 1.0, 1 / pq[1]]           # the paper's weights by hand: return, distance 1, 2, 1, 2
    for pr, wt in zip(probs, wts):
        assert abs(float(pr) - wt / sum(wts)) < 1e-6
    n = 40_000
    counts, n_fb = [0] * 5, 0
    for w in range(n):
        x, fb, zero = wr.step_ref(99, w, 1, row_v, 0, set(row_u), thr, tries=tries)
        counts[row_v.index(x)] += 1
        n_fb += fb
        assert not zero
    assert n_fb == (n if tries == 0 else 0)
    _within_5_sd(counts, probs, n)
    by_class = [[0, 0.0] for _ in range(3)]
    for x, c, pr in zip(row_v, counts, probs):
        k = wr.classify(x, 0, set(row_u))
        by_class[k][0] += c
        by_class[k][1] += float(pr)
    _within_5_sd([c for c, _ in by_class], [pr for _, pr in by_class], n)


def test_fallback_is_counted_where_it_must_occur():
    """A path 0 - 1 - 2: a step from a leaf that came from 1 has the single candidate u.  With p = 2^20 its threshold is 2^12: 64
    attempts accept it with probability 64 * 2^-20, so (at this seed) every such step takes the scan; with p = 2^40 the threshold is 0,
    W == 0, and the step is the uniform fallback.  Either way the walk goes back to 1."""
    rowptr, colidx = csr_of([(0, 1), (1, 2)], 3)
    L, n = 6, 50
    for p, want_zero in ((2.0 ** 20, 0), (2.0 ** 40, 3 * n)):
        walks, fb, zero = wr.walks_ref(rowptr, colidx, [1] * n, L, 17, p, 1.0)
        assert (walks[:, 0::2] == 1).all() and np.isin(walks[:, 1::2], (0, 2)).all()
        assert fb == 3 * n and zero == want_zero                  # steps 1, 3, 5 of every walk leave a leaf
    assert wr.walks_ref(rowptr, colidx, [1] * n, L, 17)[1:] == (0, 0)
    # p = 2^20 at vertex 1: the way back to the leaf just left is all but closed
    walks, _, _ = wr.walks_ref(rowptr, colidx, [1] * n, L, 17, 2.0 ** 20, 1.0)
    assert (walks[:, 1] != walks[:, 3]).all() and (walks[:, 3] != walks[:, 5]).all()


def test_walk_pairs_order_and_drops():
    import torch
    ops = importlib.import_module("gnncpp_amd.ops")
    walks = np.array([[0, 1, 2, 1], [3, 4, -1, -1], [5, 5, 6, 7]], dtype=np.int32)
    # offset 1: positions 0, 1, 2, walks 0, 1, 2 within each; then offset 2: positions 0, 1.  Each pair, then its reverse.
    fwd = [(0, 1), (3, 4), (5, 5), (1, 2), (5, 6), (2, 1), (6, 7),      # (4, -1) and (-1, -1) dropped
           (0, 2), (5, 6), (1, 1), (5, 7)]                               # (3, -1), (4, -1) dropped
    want_src = [v for a, b in fwd for v in (a, b)]
    want_dst = [v for a, b in fwd for v in (b, a)]
    src, dst = ops.walk_pairs(torch.from_numpy(walks), 2)
    assert src.dtype == dst.dtype == torch.int32
    assert src.tolist() == want_src and dst.tolist() == want_dst
    rs, rd = wr.pairs_ref(walks, 2)
    assert rs.tolist() == want_src and rd.tolist() == want_dst
    # a window beyond the walk adds nothing; window 0 and a walk of one position give no pair
    s5, d5 = ops.walk_pairs(torch.from_numpy(walks), 5)
    r5, _ = wr.pairs_ref(walks, 5)
    assert s5.tolist() == r5.tolist() and len(s5) > len(src)
    assert ops.walk_pairs(torch.from_numpy(walks), 0)[0].numel() == 0 and ops.walk_pairs(torch.from_numpy(walks[:, :1]), 2)[1].numel() == 0


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_header_constants_signature_and_exports(capi):
    L = capi.lib()
    assert "gnnx_csr_random_walk" in capi.declared_symbols() and hasattr(L, "gnnx_csr_random_walk")
    assert len(capi._SIGS["gnnx_csr_random_walk"]) == 14
    header = open(capi.HEADER_PATH).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (GNNX_WALK_[A-Z]+) (\d+)\s*$", header, flags=re.M)}
    assert consts["GNNX_WALK_TRIES"] == wr.TRIES == 64
    chunk = consts["GNNX_WALK_CHUNK"]
    assert 1 <= chunk <= 64 and chunk & (chunk - 1) == 0
    assert "0x77616C6B73746570" in header and "tests/walk_ref.py" in header
    csrc = os.path.join(ROOT, "gnn.cpp_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "gnnx_walk.hip" in mk and "gnnx_rng.h" in mk
    # one copy of the finaliser: the units that draw take it from the shared header
    for unit in ("gnnx_walk.hip", "gnnx_sample.hip", "gnnx_negative.hip", "gnnx_synth.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "gnnx_rng.h"' in text and "0xBF58476D1CE4E5B9" not in text, unit


def test_argument_validation_without_device(capi):
    """Validation happens before any HIP call, so these return statuses even with no GPU."""
    L = capi.lib()
    INVALID = -1
    ptr = C.c_void_p(4096)    # never dereferenced: every call below fails before a device is touched, or has nothing to do

    def walk(n_rows=4, nnz=6, rowptr=ptr, colidx=ptr, starts=ptr, n_walks=3, walk_base=0, length=5, p=1.0, q=1.0, seed=1, walks=ptr, ldw=6):
        return L.gnnx_csr_random_walk(n_rows, nnz, rowptr, colidx, starts, n_walks, walk_base, length, p, q, seed, walks, ldw, None)

    for name in ("n_rows", "nnz", "n_walks", "length", "walk_base"):
        assert walk(**{name: -1}) == INVALID, name
    assert walk(ldw=5) == INVALID and walk(length=0, ldw=0) == INVALID
    assert walk(walk_base=2 ** 32 - 2) == INVALID and walk(walk_base=2 ** 32 + 1, n_walks=0) == INVALID
    assert walk(n_walks=2 ** 32 + 1) == INVALID
    assert walk(nnz=1 << 31) == INVALID
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert walk(p=bad) == INVALID and walk(q=bad) == INVALID, bad
    for name in ("rowptr", "colidx", "starts", "walks"):
        assert walk(**{name: None}) == INVALID, name
        assert b"null" in L.gnnx_last_error()
    # valid empty results need no device: no walks (starts and walks may be null; so may colidx without entries)
    assert walk(n_walks=0, starts=None, walks=None) == 0
    assert walk(n_walks=0, nnz=0, colidx=None, starts=None, walks=None, walk_base=2 ** 32) == 0
    assert walk(n_walks=0, rowptr=None) == INVALID


def test_python_signatures():
    ops = importlib.import_module("gnncpp_amd.ops")

    def params(f):
        return list(inspect.signature(f).parameters)

    assert params(ops.random_walk) == ["rowptr", "colidx", "starts", "length", "seed", "p", "q", "walk_base", "out"]
    assert params(ops.CsrGraph.random_walk) == ["self", "starts", "length", "seed", "p", "q", "walks_per_start"]
    assert params(ops.walk_pairs) == ["walks", "window"]
    assert params(ops.EdgeSet.from_walks) == ["g", "walks", "window", "m", "seed"]
    for cls in (ops.GcnStack, ops.SageStack, ops.GatStack, ops.Gatv2Stack):
        for name in ("link_scores", "link_grad", "link_train_step", "link_evaluate"):
            assert getattr(cls, name) is getattr(ops._Stack, name), (cls.__name__, name)
        assert params(cls.grad_buffer) == ["self", "n"]
