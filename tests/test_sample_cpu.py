"""CPU checks of the neighbour sampler's restatement (tests/sample_ref.py) and of the C-ABI's argument validation: the finaliser against
synth.splitmix64, the identity on short rows, the shape of a selection, the segmented form against the direct one past the S boundary,
independence across seeds and rows, and the uniformity of the draw -- every count within 5 binomial standard deviations of its mean (a
count of n draws with probability p has mean n p and standard deviation sqrt(n p (1 - p)); 5 of them is a 6e-7 event per count)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import sample_ref as sr
from tests.helpers import ROOT, pkg, synth  # noqa: F401


def test_finaliser_is_synth_splitmix64():
    x = np.concatenate([np.arange(1000, dtype=np.uint64), np.array([2 ** 64 - 1, 2 ** 63, 0x9E3779B97F4A7C15], dtype=np.uint64),
                        np.random.default_rng(1).integers(0, 2 ** 63, 1000).astype(np.uint64) * np.uint64(2) + np.uint64(1)])
    assert np.array_equal(sr.finaliser(x), synth.splitmix64(x))
    # the key written out with Python integers for one entry: the product wraps in 64 bits
    seed, i, j = 12345, 3_000_000, 70_000
    M = sr.MASK64

    def fin(v):
        z = (v + sr.GOLDEN) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    h = fin(fin(seed) ^ ((((i << 32) | j) * sr.GOLDEN) & M))
    assert int(sr.keys(seed, i, j + 1)[j]) == ((h >> 32) << 32) | j


def test_keys_of_a_row_are_pairwise_different_and_carry_their_offset():
    u = sr.keys(7, 11, 5000)
    assert len(np.unique(u)) == 5000
    assert np.array_equal(u & np.uint64(0xFFFFFFFF), np.arange(5000, dtype=np.uint64))


def test_short_rows_are_kept_whole():
    for d, k in ((0, 1), (1, 1), (5, 5), (4, 5), (64, 64), (10, 64)):
        assert np.array_equal(sr.sample_row(3, 9, d, k), np.arange(d))
    rowptr = np.array([0, 0, 3, 8, 9], dtype=np.int32)
    colidx = np.array([4, 5, 6, 0, 1, 2, 3, 7, 2], dtype=np.int32)
    rp, ci, pos, rowid = sr.sample_ref(rowptr, colidx, 5, 1)
    assert np.array_equal(rp, rowptr) and np.array_equal(ci, colidx)
    assert np.array_equal(pos, np.arange(9)) and np.array_equal(rowid, [1, 1, 1, 2, 2, 2, 2, 2, 3])


def test_kept_positions_are_ascending_distinct_and_inside_their_row():
    rng = np.random.default_rng(5)
    deg = rng.integers(0, 40, size=60)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    colidx = rng.integers(0, 1000, size=rowptr[-1]).astype(np.int32)
    for k in (1, 7, 64):
        rp, ci, pos, rowid = sr.sample_ref(rowptr, colidx, k, 21)
        assert np.array_equal(np.diff(rp), np.minimum(deg, k))
        assert all(a.dtype == np.int32 for a in (rp, ci, pos, rowid))
        for i in range(60):
            p = pos[rp[i]:rp[i + 1]]
            assert (np.diff(p) > 0).all() and (p >= rowptr[i]).all() and (p < rowptr[i + 1]).all()
            assert (rowid[rp[i]:rp[i + 1]] == i).all()
        assert np.array_equal(ci, colidx[pos])
        # the kept entries are the k smallest keys: every kept key is below every dropped one
        i = int(np.argmax(deg))
        u = sr.keys(21, i, deg[i])
        kept = np.zeros(deg[i], dtype=bool)
        kept[pos[rp[i]:rp[i + 1]] - rowptr[i]] = True
        if k < deg[i]:
            assert u[kept].max() < u[~kept].min()


@pytest.mark.parametrize("d", [4097, 8197, 12289])
def test_segmented_form_equals_direct_form(d):
    for seed in (0, 1):
        direct = sr.sample_row(seed, 17, d, 64)
        assert len(direct) == 64
        assert np.array_equal(sr.sample_row_segmented(seed, 17, d, 64), direct)
    assert np.array_equal(sr.sample_row_segmented(2, 17, d, 5), sr.sample_row(2, 17, d, 5))
    assert np.array_equal(sr.sample_row_segmented(2, 17, d, 5, S=100), sr.sample_row(2, 17, d, 5))


def test_a_different_seed_or_row_gives_a_different_set():
    a = sr.sample_row(1, 5, 200, 20)
    assert not np.array_equal(a, sr.sample_row(2, 5, 200, 20))
    assert not np.array_equal(a, sr.sample_row(1, 6, 200, 20))
    assert np.array_equal(a, sr.sample_row(1, 5, 200, 20))
    assert not np.array_equal(a, sr.sample_row(1 + 2 ** 32, 5, 200, 20))     # all 64 bits of the seed count


def worst_sd(counts, n, p):
    p = np.asarray(p, dtype=np.float64)
    return float((np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))).max())


@pytest.mark.parametrize("d,k", [(40, 10), (65, 64)])
def test_uniform_over_seeds(d, k):
    n = 4000
    counts = np.zeros(d)
    for seed in range(n):
        counts[sr.sample_row(seed, 3, d, k)] += 1
    w = worst_sd(counts, n, k / d)
    print(f"(d, k) = ({d}, {k}), {n} seeds: largest deviation {w:.2f} sd")
    assert w <= 5.0


def test_uniform_over_rows_at_one_seed():
    n, d, k = 4000, 40, 10
    counts = np.zeros(d)
    for i in range(n):
        counts[sr.sample_row(77, i, d, k)] += 1
    w = worst_sd(counts, n, k / d)
    print(f"(d, k) = ({d}, {k}), {n} rows at one seed: largest deviation {w:.2f} sd")
    assert w <= 5.0


def test_uniform_over_the_segments_of_a_hub_row():
    n, d, k = 2000, 9000, 5
    lens = np.array([4096, 4096, 808])
    counts = np.zeros(3)
    for seed in range(n):
        counts += np.bincount(sr.sample_row(seed, 123, d, k) // sr.SEG, minlength=3)
    w = worst_sd(counts, n * k, lens / d)
    print(f"d = {d}, k = {k}, {n} seeds, per segment: largest deviation {w:.2f} sd")
    assert w <= 5.0


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_argument_validation_without_device(capi):
    """Validation happens before any HIP call, so these return statuses even with no GPU."""
    L = capi.lib()
    INVALID, UNSUPPORTED = -1, -7
    assert hasattr(L, "gnnx_csr_sample_workspace") and hasattr(L, "gnnx_csr_sample_neighbors")
    assert L.gnnx_version() == 100
    b = C.c_size_t(0)

    def query(n_rows, nnz, k):
        assert L.gnnx_csr_sample_workspace(n_rows, nnz, k, C.byref(b)) == 0
        return b.value

    def formula(n_rows, nnz, k, S=4096):
        tiles, hubs = n_rows // 1024 + 1, min(nnz // (S + 1), n_rows)
        segs, longs = nnz // S + hubs, min(nnz // 257, n_rows)
        return 256 + -(-4 * (16 + tiles + 2 * hubs + segs + segs * k + longs) // 256) * 256          # the header's formula

    for shape in ((1000, 5000, 10), (1000, 10_000_000, 10), (1000, 10_000_000, 25), (1000, 100_000_000, 25), (10_000_000, 100_000_000, 64),
                  (0, 0, 1), (5, 4096, 3), (5, 4097, 3)):
        assert query(*shape) == formula(*shape), shape
    assert query(1000, 10_000_000, 10) > query(1000, 5000, 10)                     # grows with nnz
    assert query(1000, 10_000_000, 25) > query(1000, 10_000_000, 10)               # and with k
    assert L.gnnx_csr_sample_workspace(1000, 5000, 10, None) == INVALID
    assert L.gnnx_csr_sample_workspace(-1, 5000, 10, C.byref(b)) == INVALID
    assert L.gnnx_csr_sample_workspace(1000, -1, 10, C.byref(b)) == INVALID
    assert L.gnnx_csr_sample_workspace(1000, 1 << 31, 10, C.byref(b)) == INVALID
    assert L.gnnx_csr_sample_workspace(1000, 5000, 0, C.byref(b)) == INVALID
    assert L.gnnx_csr_sample_workspace(1000, 5000, 65, C.byref(b)) == UNSUPPORTED
    p = C.c_void_p(4096)    # never dereferenced: every call below fails before a device is touched
    nnz_out = C.c_int64(-5)

    def sample(n_rows=4, nnz=6, rowptr=p, colidx=p, k=3, seed=1, rowptr_out=p, colidx_out=p, pos=None, rowid=None, cap=6, out=C.byref(nnz_out),
               ws=p, wsb=1 << 20):
        return L.gnnx_csr_sample_neighbors(n_rows, nnz, rowptr, colidx, k, seed, rowptr_out, colidx_out, pos, rowid, cap, out, ws, wsb, None)

    assert sample(k=0) == INVALID and sample(k=-3) == INVALID
    assert sample(k=65) == UNSUPPORTED
    for name in ("rowptr", "colidx", "rowptr_out", "colidx_out", "out"):
        assert sample(**{name: None}) == INVALID, name
        assert b"null" in L.gnnx_last_error()
    for name in ("n_rows", "nnz", "cap"):
        assert sample(**{name: -1}) == INVALID, name
    assert sample(nnz=1 << 31) == INVALID
    assert sample(ws=None) == -4 and sample(wsb=16) == -4
    assert nnz_out.value == -5          # a refused call writes nothing
