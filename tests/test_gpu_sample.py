"""GPU tests of the neighbour sampler (run with -m gpu on an MI355X): gnnx_csr_sample_neighbors through ops.sample_neighbors and
CsrGraph.sample_neighbors.  The sampler is integer work with one right answer: every output -- rowptr', colidx', pos, rowid -- is
compared with tests/sample_ref.py by array_equal.  Cases: a crafted CSR whose row lengths sit around every k used, at the S = 4096
boundary and on hub rows whose last segment is shorter than k; rows around L = 256, where a row leaves the row kernel for a wavefront of
its own; every lane-group width the row kernel can pick; the R-MAT
graph of tests/test_gpu_sage.py (empty rows, rows longer than 64); the statuses that can only be seen with a device."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests.helpers import synth
from tests.reduce_ref import transpose_csr
from tests.sample_ref import sample_ref

pytestmark = pytest.mark.gpu

N, E = 1 << 10, 8000
CRAFTED = [0, 1, 4, 5, 6, 15, 16, 17, 63, 64, 65, 100, 0, 4095, 4096, 4097, 8192, 8197, 12289, 3]
N_COLS = 16384
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
    return None if t is None else t.detach().cpu().numpy()


def csr_of_lengths(lengths, n_cols, seed):
    """A CSR with the given row lengths; a row's columns are a prefix of a seeded permutation of [0, n_cols), sorted."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.permutation(n_cols)[:d]) for d in lengths]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


def assert_is_reference(env, rowptr, colidx, k, seed, what):
    got = env["ops"].sample_neighbors(dev(env, rowptr), dev(env, colidx), k, seed, want_pos=True, want_rowid=True)
    ref = sample_ref(rowptr, colidx, k, seed)
    for name, g, r in zip(("rowptr", "colidx", "pos", "rowid"), got, ref):
        g = host(g)
        assert g.dtype == np.int32 and np.array_equal(g, r), f"{what}: {name} differs from the reference"
    return got


@pytest.fixture(scope="module")
def crafted():
    rowptr, colidx = csr_of_lengths(CRAFTED, N_COLS, seed=41)
    assert rowptr[-1] // len(CRAFTED) > 32            # the widest lane group
    return rowptr, colidx


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF12345678])
@pytest.mark.parametrize("k", [1, 5, 16, 63, 64])
def test_crafted_rows_vs_reference(env, crafted, k, seed):
    """Lengths around every k (0 / 1, 4 / 5 / 6, 15 / 16 / 17, 63 / 64 / 65), 4095 / 4096 / 4097 around S, a hub of two full segments
    (8192) and hubs whose last segment is shorter than k: 4097 and 12289 (1 entry), 8197 (5 entries)."""
    rowptr, colidx = crafted
    assert_is_reference(env, rowptr, colidx, k, seed, f"k = {k}")


@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_rows_around_the_long_row_threshold(env, width):
    """Rows of more than L = 256 and at most S entries leave the row kernel for a wavefront of their own: lengths on both sides of L and
    up to S, among short rows, with lane groups of 4 (many empty rows bring the mean down) and of 64."""
    lengths = [255, 256, 257, 258, 0, 300, 40, 511, 1023, 7, 2000, 4096, 257, 3]
    if width == "narrow":
        lengths = lengths + [0] * 3000
    rowptr, colidx = csr_of_lengths(lengths, N_COLS, seed=43)
    assert (int(rowptr[-1]) // len(lengths) <= 4) == (width == "narrow") and (int(rowptr[-1]) // len(lengths) > 32) == (width == "wide")
    for k in (5, 64):
        assert_is_reference(env, rowptr, colidx, k, 77, f"{width}, k = {k}")


@pytest.mark.parametrize("mean,lanes", [(3, 4), (7, 8), (14, 16), (28, 32), (60, 64)])
def test_every_lane_group_width(env, mean, lanes):
    """The row kernel gives a row 4 .. 64 lanes by the mean row length (more than 32: 64, more than 16: 32, more than 8: 16, more than 4: 8,
    else 4); the result must not depend on it.  300 rows of 0 .. 2 * mean entries, three of them of several windows of any width."""
    rng = np.random.default_rng(100 + mean)
    lengths = rng.integers(0, 2 * mean + 1, size=300)
    lengths[[7, 150, 299]] = [200, 131, 64 + mean]
    rowptr, colidx = csr_of_lengths(lengths, 2048, seed=mean)
    m = int(rowptr[-1]) // 300
    assert (64 if m > 32 else 32 if m > 16 else 16 if m > 8 else 8 if m > 4 else 4) == lanes
    for k in (5, 16):
        assert_is_reference(env, rowptr, colidx, k, 9, f"mean {mean}, k = {k}")


@pytest.fixture(scope="module")
def task(env):
    ops = env["ops"]
    src, dst = synth.rmat_edges(91, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    deg = np.diff(rowptr)
    assert (deg == 0).any() and deg.max() > 64
    return dict(g=g, src=src, dst=dst, rowptr=rowptr, colidx=colidx, deg=deg)


@pytest.mark.parametrize("k", [5, 25])
def test_rmat_vs_reference_and_repeats(env, task, k):
    ops, torch = env["ops"], env["torch"]
    first = assert_is_reference(env, task["rowptr"], task["colidx"], k, 2024, f"R-MAT, k = {k}")
    again = ops.sample_neighbors(task["g"].rowptr, task["g"].colidx, k, 2024, want_pos=True, want_rowid=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    bare = ops.sample_neighbors(task["g"].rowptr, task["g"].colidx, k, 2024)
    assert bare[2] is None and bare[3] is None
    assert torch.equal(bare[0], first[0]) and torch.equal(bare[1], first[1])
    other = ops.sample_neighbors(task["g"].rowptr, task["g"].colidx, k, 2025)
    assert torch.equal(other[0], first[0]) and not torch.equal(other[1], first[1])


def raw_call(env, rowptr, colidx, k, seed, cap, ws_bytes=None, n_rows=None):
    """The C call on sentinel-filled outputs -> (status, nnz_out, rowptr', colidx', pos, rowid)."""
    torch, capi = env["torch"], env["capi"]
    L = capi.lib()
    n_rows = int(rowptr.numel()) - 1 if n_rows is None else n_rows
    nnz = int(colidx.numel())
    need = C.c_size_t(0)
    assert L.gnnx_csr_sample_workspace(n_rows, nnz, k, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=env["dev"])
    outs = [torch.full((n,), SENTINEL, dtype=torch.int32, device=env["dev"]) for n in (n_rows + 1, max(cap, 1), max(cap, 1), max(cap, 1))]
    nnz_out = C.c_int64(-1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = L.gnnx_csr_sample_neighbors(n_rows, nnz, p(rowptr), p(colidx), k, seed, *(p(t) for t in outs), cap, C.byref(nnz_out), p(ws),
                                     need.value if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return (st, nnz_out.value, *outs)


def test_statuses_with_a_device(env, task):
    g, k = task["g"], 5
    kept = int(np.minimum(task["deg"], k).sum())
    st, nnz_out, rp, ci, pos, rowid = raw_call(env, g.rowptr, g.colidx, k, 1, kept)
    assert st == 0 and nnz_out == kept and int(rp[-1]) == kept and not bool((ci == SENTINEL).any())
    st, nnz_out, *outs = raw_call(env, g.rowptr, g.colidx, k, 1, kept - 1)        # one short: refused whole, the count still reported
    assert st == -1 and nnz_out == kept
    assert b"nnz_capacity" in env["capi"].lib().gnnx_last_error()
    for t in outs:
        assert bool((t == SENTINEL).all())
    need = C.c_size_t(0)
    assert env["capi"].lib().gnnx_csr_sample_workspace(N, g.nnz, k, C.byref(need)) == 0
    st, nnz_out, *outs = raw_call(env, g.rowptr, g.colidx, k, 1, kept, ws_bytes=need.value - 1)
    assert st == -4 and nnz_out == -1
    for t in outs:
        assert bool((t == SENTINEL).all())
    st, nnz_out, rp, *rest = raw_call(env, g.rowptr[:1], g.colidx[:0], k, 1, 0)    # no rows
    assert st == 0 and nnz_out == 0 and host(rp).tolist() == [0]
    with pytest.raises(env["capi"].GnnxError):
        env["ops"].sample_neighbors(g.rowptr, g.colidx, 65, 1)
    with pytest.raises(env["capi"].GnnxError):
        env["ops"].sample_neighbors(g.rowptr, g.colidx, 0, 1)


def test_graph_sample(env, task):
    ops, torch, capi, g = env["ops"], env["torch"], env["capi"], task["g"]
    k, seed = 5, 31
    gs = g.sample_neighbors(k, seed)
    rp, ci, _, rowid = sample_ref(task["rowptr"], task["colidx"], k, seed)
    assert gs.n == N and gs.nnz == len(ci) and gs.nid is None and gs.plan is None
    assert np.array_equal(host(gs.rowptr), rp) and np.array_equal(host(gs.colidx), ci)
    rp_t, ci_t, map_t = transpose_csr(rp, ci, N)
    assert np.array_equal(host(gs.rowptr_t), rp_t) and np.array_equal(host(gs.colidx_t), ci_t)
    # the parent has neither self loops nor duplicates, so the reference build of the sampled COO is the sample itself
    built = ops.CsrGraph.from_coo(dev(env, rowid), dev(env, ci), N)
    assert torch.equal(built.rowptr, gs.rowptr) and torch.equal(built.colidx, gs.colidx)
    assert torch.equal(built.rowptr_t, gs.rowptr_t) and torch.equal(built.colidx_t, gs.colidx_t)
    assert torch.equal(built.s, gs.s) and torch.equal(built.norm, gs.norm)
    assert np.array_equal(host(gs.attention_map()), map_t)
    bare = g.sample_neighbors(k, seed, transpose=False, norm=False)
    assert bare.rowptr_t is None and bare.norm is None and torch.equal(bare.colidx, gs.colidx)
    with_plans = ops.CsrGraph.from_coo(dev(env, task["src"]), dev(env, task["dst"]), N)
    with_plans.make_plans(64, 32)
    planned = with_plans.sample_neighbors(k, seed)
    assert planned.plan is not None and planned.plan_t is not None and planned._plan_args == with_plans._plan_args
    assert torch.equal(planned.colidx, gs.colidx)
    moved = ops.CsrGraph.from_coo(dev(env, task["src"]), dev(env, task["dst"]), N, relabel="scramble")
    with pytest.raises(capi.GnnxError, match="relabel") as info:
        moved.sample_neighbors(k, seed)
    assert info.value.status == -7
