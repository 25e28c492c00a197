"""GPU tests of the listed-row sampler (run with -m gpu on an MI355X): gnnx_csr_sample_rows through ops.sample_rows and the raw C
call, and gnnx_csr_renumber_cols.  Integer work with one right answer: rowptr', colidx', pos, rowid and the column mark are compared
by array_equal with tests/sample_ref.py's whole-graph sample cut to the listed rows, and with the rows of the device's own whole-graph
call.  One crafted CSR has a row in every length class of the kernels (copy, group select, long-row list, two- and three-segment
hubs, an empty row); five uniform graphs reach every lane-group width; the whole-graph call is held to the reference on the same
graphs, so the kernels it shares with the listed call kept their bits."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests.helpers import pkg  # noqa: F401  (registers the package under its importable alias)
from tests.sample_ref import sample_ref

pytestmark = pytest.mark.gpu

N_COLS = 10000
SENTINEL = -77


def lengths_for(k):
    return [0, 1, k - 1, k, k + 1, 64, 65, 256, 257, 1000, 4096, 4097, 8193, 9000]


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


def cut(ref, rows, n_cols):
    """(rowptr', colidx', pos, rowid, mark) of a row list from the whole-graph sample `ref`."""
    rp, ci, pos, _ = ref
    lens = [int(rp[i + 1] - rp[i]) for i in rows]
    take = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in rows]).astype(np.int64) if len(rows) else np.zeros(0, dtype=np.int64)
    mark = np.zeros(n_cols, dtype=np.uint8)
    mark[ci[take]] = 1
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), ci[take], pos[take],
            np.repeat(np.arange(len(rows), dtype=np.int32), lens), mark)


def assert_listed(env, d_rowptr, d_colidx, ref, rows, n_cols, k, seed, what, whole=None):
    torch = env["torch"]
    mark = torch.zeros(n_cols, dtype=torch.uint8, device=env["dev"])
    got = env["ops"].sample_rows(d_rowptr, d_colidx, dev(env, np.asarray(rows, dtype=np.int32)), k, seed, n_cols=n_cols, want_pos=True,
                                 want_rowid=True, col_mark=mark)
    want = cut(ref, rows, n_cols)
    for name, g, r in zip(("rowptr", "colidx", "pos", "rowid", "mark"), (*got, mark), want):
        g = host(g)
        assert g.dtype == r.dtype and np.array_equal(g, r), f"{what}: {name} differs from the reference"
    if whole is not None:        # and the rows of the device's own whole-graph call
        for name, g, r in zip(("rowptr", "colidx", "pos", "rowid"), got, cut(tuple(host(t) for t in whole), rows, n_cols)):
            assert np.array_equal(host(g), r), f"{what}: {name} differs from the whole-graph call"


@pytest.mark.parametrize("k", [1, 5, 64])
def test_every_length_class_and_list_shape(env, k):
    lengths = lengths_for(k)
    rowptr, colidx = csr_of_lengths(lengths, N_COLS, seed=50 + k)
    n, seed = len(lengths), 0xC0FFEE + k
    assert int(rowptr[-1]) // n > 32
    ref = sample_ref(rowptr, colidx, k, seed)
    d_rowptr, d_colidx = dev(env, rowptr), dev(env, colidx)
    whole = env["ops"].sample_neighbors(d_rowptr, d_colidx, k, seed, want_pos=True, want_rowid=True)
    for name, g, r in zip(("rowptr", "colidx", "pos", "rowid"), whole, ref):
        assert np.array_equal(host(g), r), f"whole graph: {name} differs from the reference"
    lists = {"all rows": list(range(n)), "reversed": list(range(n))[::-1], "empty": [],
             "one repeated row": [3, 12, 9, 12, 0, 12], "a repeated row and others twice": [13, 5, 13, 7, 5, 10, 8, 11]}
    for i, d in enumerate(lengths):
        lists[f"the row of {d} alone"] = [i]
    # more repeats of long rows than the lists of long rows hold (8 hubs, about 140 long rows here): the lane group's own selection
    lists["long rows past their lists"] = [12] * 10 + [9] * 150 + [13]
    for what, rows in lists.items():
        assert_listed(env, d_rowptr, d_colidx, ref, rows, N_COLS, k, seed, f"k = {k}, {what}", whole)
    bare = env["ops"].sample_rows(d_rowptr, d_colidx, dev(env, np.array([12, 4], dtype=np.int32)), k, seed, n_cols=N_COLS)
    assert bare[2] is None and bare[3] is None and np.array_equal(host(bare[1]), cut(ref, [12, 4], N_COLS)[1])


@pytest.mark.parametrize("mean,lanes", [(3, 4), (6, 8), (12, 16), (24, 32), (48, 64)])
def test_every_lane_group_width(env, mean, lanes):
    """256 rows whose mean length is exactly `mean` (pairs of mean + d and mean - d entries), k = 2, every third row listed."""
    rng = np.random.default_rng(200 + mean)
    delta = rng.integers(0, mean + 1, size=128)
    lengths = np.stack([mean + delta, mean - delta], 1).reshape(-1)
    rowptr, colidx = csr_of_lengths(lengths, 1024, seed=mean)
    m = int(rowptr[-1]) // 256
    assert m == mean and (64 if m > 32 else 32 if m > 16 else 16 if m > 8 else 8 if m > 4 else 4) == lanes
    k, seed = 2, 17
    ref = sample_ref(rowptr, colidx, k, seed)
    d_rowptr, d_colidx = dev(env, rowptr), dev(env, colidx)
    whole = env["ops"].sample_neighbors(d_rowptr, d_colidx, k, seed, want_pos=True, want_rowid=True)
    for name, g, r in zip(("rowptr", "colidx", "pos", "rowid"), whole, ref):
        assert np.array_equal(host(g), r), f"mean {mean}, whole graph: {name} differs from the reference"
    assert_listed(env, d_rowptr, d_colidx, ref, list(range(0, 256, 3)), 1024, k, seed, f"mean {mean}", whole)


def raw_call(env, rowptr, colidx, rows, k, seed, cap, ws_bytes=None, n_cols=N_COLS):
    """The C call on sentinel-filled outputs and a zeroed mark -> (status, nnz_out, rowptr', colidx', pos, rowid, mark)."""
    torch, L = env["torch"], env["capi"].lib()
    n_rows, nnz, m = int(rowptr.numel()) - 1, int(colidx.numel()), int(rows.numel())
    need = C.c_size_t(0)
    kq = min(max(k, 1), 64)        # the query refuses the fanouts the call is asked to refuse
    assert L.gnnx_csr_sample_workspace(m, nnz, kq, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=env["dev"])
    outs = [torch.full((n,), SENTINEL, dtype=torch.int32, device=env["dev"]) for n in (m + 1, max(cap, 1), max(cap, 1), max(cap, 1))]
    mark = torch.zeros(n_cols, dtype=torch.uint8, device=env["dev"])
    nnz_out = C.c_int64(-1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = L.gnnx_csr_sample_rows(n_rows, n_cols, nnz, p(rowptr), p(colidx), p(rows), m, k, seed, *(p(t) for t in outs), p(mark), cap,
                                C.byref(nnz_out), p(ws), need.value if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return (st, nnz_out.value, *outs, mark)


def untouched(outs, mark):
    return all(bool((t == SENTINEL).all()) for t in outs) and not bool(mark.any())


def test_statuses(env):
    k = 5
    lengths = lengths_for(k)
    rowptr, colidx = csr_of_lengths(lengths, N_COLS, seed=50 + k)
    d_rowptr, d_colidx = dev(env, rowptr), dev(env, colidx)
    rows = np.array([13, 2, 6, 1], dtype=np.int32)
    kept = int(np.minimum(np.asarray(lengths)[rows], k).sum())
    last_error = env["capi"].lib().gnnx_last_error
    st, nnz_out, rp, ci, pos, rowid, mark = raw_call(env, d_rowptr, d_colidx, dev(env, rows), k, 1, kept)
    assert st == 0 and nnz_out == kept and int(rp[-1]) == kept and not bool((ci == SENTINEL).any()) and int(mark.sum()) > 0
    for bad in (-1, len(lengths)):                                   # an id outside [0, n_rows): nothing written
        st, nnz_out, *outs, mark = raw_call(env, d_rowptr, d_colidx, dev(env, np.array([13, bad, 6], dtype=np.int32)), k, 1, 64)
        assert st == -3 and untouched(outs, mark), bad
        assert b"outside" in last_error()
        with pytest.raises(env["capi"].GnnxError) as info:
            env["ops"].sample_rows(d_rowptr, d_colidx, dev(env, np.array([bad], dtype=np.int32)), k, 1)
        assert info.value.status == -3
    st, nnz_out, *outs, mark = raw_call(env, d_rowptr, d_colidx, dev(env, rows), k, 1, kept - 1)   # one short: the count still reported
    assert st == -1 and nnz_out == kept and untouched(outs, mark)
    assert b"nnz_capacity" in last_error()
    st, nnz_out, *outs, mark = raw_call(env, d_rowptr, d_colidx, dev(env, rows), 0, 1, kept)
    assert st == -1 and untouched(outs, mark)
    st, nnz_out, *outs, mark = raw_call(env, d_rowptr, d_colidx, dev(env, rows), 65, 1, kept)
    assert st == -7 and untouched(outs, mark)
    need = C.c_size_t(0)
    assert env["capi"].lib().gnnx_csr_sample_workspace(len(rows), int(rowptr[-1]), k, C.byref(need)) == 0
    st, nnz_out, *outs, mark = raw_call(env, d_rowptr, d_colidx, dev(env, rows), k, 1, kept, ws_bytes=need.value - 1)
    assert st == -4 and nnz_out == -1 and untouched(outs, mark)
    for k_bad in (0, 65):
        with pytest.raises(env["capi"].GnnxError):
            env["ops"].sample_rows(d_rowptr, d_colidx, dev(env, rows), k_bad, 1)


def test_renumber_cols(env):
    ops, torch = env["ops"], env["torch"]
    below = np.array([2, 3, 7, 11, 400], dtype=np.int32)
    pos = ops.rows_to_positions(dev(env, below), 500)
    ci = np.array([400, 2, 2, 11, 7, 3, 400], dtype=np.int32)
    got = ops.renumber_cols(dev(env, ci), pos)
    assert np.array_equal(host(got), np.searchsorted(below, ci).astype(np.int32))
    for bad in (5, 500, -1):                                         # no position / outside the table: refused, never a wrong index
        t = dev(env, np.array([400, bad, 2], dtype=np.int32))
        with pytest.raises(env["capi"].GnnxError) as info:
            ops.renumber_cols(t, pos)
        assert info.value.status == -3 and host(t).tolist() == [4, -1, 0]
    empty = torch.empty(1, dtype=torch.int32, device=env["dev"])[:0]
    assert ops.renumber_cols(empty, pos).numel() == 0
