"""GPU tests of the graph readout (run with -m gpu on an MI355X): ops.segment_pool / ops.segment_pool_bwd against tests/pool_ref.py, bit
for bit in value and arg, on the segment table and the values of tests/pool_ref.py (about 20 000 rows; tests/test_pool_ref_cpu.py shows
that they tell the contract's order from its neighbours).

Dispatch cells of gnnx_pool.hip (shape_of): VEC in {4, 1} x G in {4, 8, 16, 32, 64} lanes per tile x one or several feature tiles, the
forward kernel in a summing (SUM, MEAN) and a comparing (MAX) form, the backward in one form per op; a combine kernel whenever
n_rows > T, which takes the chunk partials of a long segment in two batch forms: 64 at once while at least 64 chunks are left (so only
a segment of 65 chunks or more, 64 T + 1 rows, reaches it) and up to 8 at once behind that.  The shared table's longest segment has 41
chunks and takes the 8-wide form only; test_combine_takes_64_partials_at_once runs segments of 65, 71 and 130 chunks for the 64-wide
form alone, followed by the 8-wide one, and taken twice.  The issue's widths 1, 3, 4, 5, 16, 20, 64, 68, 128, 132, 256, 260, 516 cover the 16-byte cells G = 4 (4, 16), 8 (20),
16 (64), 32 (68, 128), 64 (132, 256), two tiles (260) and three (516), and the scalar cells G = 4 (1, 3) and 8 (5).  They miss the
scalar cells G = 16 (9 .. 16 features), G = 32 (17 .. 32) and the scalar kernel on several tiles (more than 64 features): 13, 29 and 67
are added for those (the misaligned F = 64 layouts are the scalar G = 64 cell on one tile).  Every width runs every op, forward and
backward, both betas."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from tests import pool_ref
from tests.helpers import pkg  # noqa: F401  (registers the in-tree package under its importable alias)
from tests.pool_ref import T, pool_bwd

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 13, 16, 20, 29, 64, 67, 68, 128, 132, 256, 260, 516)
LAYOUTS = ("x_off", "x_ld", "y_off", "y_ld", "arg_off", "arg_ld", "g_off", "g_ld", "dx_off", "dx_ld")   # at F = 64, one at a time
ARG_FILL = -777


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    e = dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))
    e["segptr"] = torch.from_numpy(table()).to(e["dev"])      # the table's properties are asserted before the first GPU call
    return e


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def table():
    """segment_table() with the properties this file relies on asserted."""
    segptr = pool_ref.segment_table()
    sp = segptr.astype(np.int64)
    lens = np.diff(sp)
    assert segptr.dtype == np.int32 and sp[0] == 0 and (lens >= 0).all() and 18_000 <= sp[-1] <= 22_000
    assert lens[0] == 0 and lens[-1] == 0 and any((lens[i:i + 3] == 0).all() for i in range(len(lens) - 2))
    for ln in (1, 2, 63, 64, 65) + pool_ref.LONG:
        assert (lens == ln).any(), ln
    run = best = 0
    for v in (lens >= 1) & (lens <= 3):
        run = run + 1 if v else 0
        best = max(best, run)
    assert best >= 300
    long_b = np.nonzero(lens > T)[0]
    assert len(long_b) >= 7
    for b in np.nonzero(lens >= T - 1)[0][:len(pool_ref.LONG)]:
        assert 0 < lens[b - 1] < T and 0 < lens[b + 1] < T
    mixed = False   # a global tile with the tail of one long segment, whole short ones and the head of another
    for t in range(int(sp[-1]) // T + 1):
        lo, hi = t * T, (t + 1) * T
        tails = any(sp[b] < lo < sp[b + 1] <= hi for b in long_b)
        heads = any(lo < sp[b] < hi < sp[b + 1] for b in long_b)
        whole = any(0 < lens[b] <= T and lo <= sp[b] and sp[b + 1] <= hi for b in range(len(lens)))
        mixed |= tails and heads and whole
    assert mixed
    return segptr


def values(op, F):
    return (pool_ref.max_values() if op == "max" else pool_ref.sum_values())[:, :F]


@functools.lru_cache(maxsize=None)
def bwd_reference(op, beta):
    """The contract's dX at the widest width, computed once per (op, beta); a narrower width is its leading columns."""
    G, dX0 = pool_ref.grad_values()
    arg = pool_ref.reference("max")[1] if op == "max" else None
    d = pool_bwd(table(), G, op, arg=arg, dX=dX0 if beta else None, beta=beta)
    d.setflags(write=False)
    return d


def strided(env, rows, F, dtype, fill, ld=None, off=0):
    """A [rows, F] view on leading dimension ld, `off` elements into its buffer; the whole buffer -- pad columns, the elements in front
    of the view and a row's worth behind it -- set to `fill`."""
    torch = env["torch"]
    ld = F if ld is None else ld
    buf = torch.full((off + (rows + 1) * ld,), fill, dtype=dtype, device=env["dev"])
    return torch.as_strided(buf, (rows, F), (ld, 1), off), buf


def placed(env, a, ld=None, off=0):
    view, buf = strided(env, a.shape[0], a.shape[1], env["torch"].from_numpy(a[:1]).dtype, 0, ld, off)
    view.copy_(dev(env, a))
    return view


def untouched_outside(env, view, buf, fill, what):
    """Every element of buf outside the view still holds `fill` (NaN for float buffers)."""
    torch = env["torch"]
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    rows, F = view.shape
    off, ld = view.storage_offset() - buf.storage_offset(), view.stride(0)
    if rows and F:
        idx = off + (torch.arange(rows, device=buf.device) * ld)[:, None] + torch.arange(F, device=buf.device)[None, :]
        keep[idx.reshape(-1)] = False
    outside = buf[keep]
    ok = torch.isnan(outside).all() if fill != fill else (outside == fill).all()
    assert bool(ok), f"{what}: an element outside the matrix was written"


def run(env, F, layout="aligned"):
    """Every op at width F: the forward's value and arg, the backward with beta = 0 into a NaN-filled dX and with beta = 1."""
    ops, torch = env["ops"], env["torch"]
    segptr = env["segptr"]
    n_seg, n_rows = len(table()) - 1, int(table()[-1])
    G, dX0 = pool_ref.grad_values()
    nan = float("nan")

    def geometry(name):   # (ld, off) of matrix `name` under this layout
        return (F + 1 if layout == name + "_ld" else None, 1 if layout == name + "_off" else 0)

    d_G = placed(env, G[:, :F], *geometry("g"))
    for op in pool_ref.OPS:
        what = f"F={F} {layout} {op}"
        d_X = placed(env, values(op, F), *geometry("x"))
        Y, Ybuf = strided(env, n_seg, F, torch.float32, nan, *geometry("y"))
        arg, argbuf = strided(env, n_seg, F, torch.int32, ARG_FILL, *geometry("arg"))
        Yo, argo = ops.segment_pool(segptr, d_X, op, out=Y, arg_out=arg)
        Yr, argr = pool_ref.reference(op)
        assert Yo is Y and np.array_equal(bits(host(Y)), bits(Yr[:, :F])), what
        untouched_outside(env, Y, Ybuf, nan, what + " Y")
        if op == "max":
            assert argo is arg and np.array_equal(host(arg), argr[:, :F]), what
            untouched_outside(env, arg, argbuf, ARG_FILL, what + " arg")
            Y2, none = ops.segment_pool(segptr, d_X, op, want_arg=False)               # without the arg: the same values
            assert none is None and np.array_equal(bits(host(Y2)), bits(Yr[:, :F])), what
        else:
            assert argo is None and bool((argbuf == ARG_FILL).all()), what + ": SUM and MEAN never write arg"
            arg = None
        for beta in (0.0, 1.0):
            dX, dXbuf = strided(env, n_rows, F, torch.float32, nan, *geometry("dx"))
            if beta:
                dX.copy_(dev(env, dX0[:, :F]))
            out = ops.segment_pool_bwd(segptr, d_G, op, arg=arg, out=dX, beta=beta)
            got = host(dX)
            assert out is dX and not np.isnan(got).any(), what + f" beta={beta}: NaN left in dX"
            assert np.array_equal(bits(got), bits(bwd_reference(op, beta)[:, :F])), what + f" beta={beta}"
            untouched_outside(env, dX, dXbuf, nan, what + " dX")


@pytest.mark.parametrize("F", WIDTHS)
def test_bits_of_every_op_forward_and_backward(env, F):
    run(env, F)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bits_do_not_change_off_16_byte_alignment(env, layout):
    run(env, 64, layout)


def test_position_independence(env):
    """Every segment pooled alone, as a one-segment call on its own rows, has the bits it has in the batch."""
    ops, torch = env["ops"], env["torch"]
    F = 68
    sp = table().astype(np.int64)
    n_seg = len(sp) - 1
    one = {}
    for op in pool_ref.OPS:
        d_X = dev(env, values(op, F))
        Y = torch.full((n_seg, F), float("nan"), dtype=torch.float32, device=env["dev"])
        arg = torch.full((n_seg, F), ARG_FILL, dtype=torch.int32, device=env["dev"])
        for b in range(n_seg):
            s, e = int(sp[b]), int(sp[b + 1])
            ptr = one.get(e - s)
            if ptr is None:
                ptr = one[e - s] = dev(env, np.array([0, e - s], dtype=np.int32))
            ops.segment_pool(ptr, d_X[s:e], op, out=Y[b:b + 1], arg_out=arg[b:b + 1])
        Yr, argr = pool_ref.reference(op)
        assert np.array_equal(bits(host(Y)), bits(Yr[:, :F])), op
        if op == "max":
            rel = np.where(argr[:, :F] >= 0, argr[:, :F] - sp[:-1, None], -1)       # rows count from the slice's own first row
            assert np.array_equal(host(arg), rel), op


@functools.lru_cache(maxsize=None)
def long_case():
    """(segptr, X for sum and mean, X for max) with segments of 65 T (the 64-wide batch alone), 70 T + 3 (one 64-wide batch, then 6 chunks
    in the 8-wide form, the last of 3 rows) and 129 T + 9 (two 64-wide batches and one chunk), short segments between them; F = 12."""
    F = 12
    lens = [5, 65 * T, 3, 70 * T + 3, 0, 1, 129 * T + 9, 2]
    segptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(segptr[-1])
    rng = np.random.default_rng(99)
    Xs = (rng.choice([-1.0, 1.0], size=(n, F)) * rng.uniform(1.0, 2.0, size=(n, F)) * np.exp2(rng.integers(-12, 13, size=(n, F)))).astype(np.float32)
    Xm = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], dtype=np.float32)[rng.integers(0, 6, size=(n, F))]
    # winners beyond chunk 64: every third column holds the lowest value up to chunk 66 of the second long segment and chunk 128 of the
    # third; every third column + 1 holds only ties (the first row must win through every batch)
    for b, first in ((3, 66 * T + 5), (6, 128 * T + 1)):
        Xm[segptr[b]:segptr[b] + first, 0::3] = -2.0
    Xm[:, 1::3] = 1.0
    return segptr, Xs, Xm


def test_combine_takes_64_partials_at_once(env):
    ops = env["ops"]
    segptr, Xs, Xm = long_case()
    sp = segptr.astype(np.int64)
    chunks = -(-np.diff(sp) // T)
    assert sorted(chunks[chunks > 64].tolist()) == [65, 71, 130]
    d_ptr = dev(env, segptr)
    for op in pool_ref.OPS:
        X = Xm if op == "max" else Xs
        Yr, argr = pool_ref.pool_fwd(segptr, X, op)
        Y, arg = ops.segment_pool(d_ptr, dev(env, X), op)
        assert np.array_equal(bits(host(Y)), bits(Yr)), op
        if op == "max":
            assert np.array_equal(host(arg), argr)
            assert (argr[3, 0::3] >= sp[3] + 64 * T).all() and (argr[6, 0::3] >= sp[6] + 128 * T).all()   # winners beyond chunk 64
            assert (argr[[1, 3, 6], 1::3] == sp[[1, 3, 6], None]).all()                                  # all ties: the first row
            G = pool_ref.grad_values()[0][:len(sp) - 1, :X.shape[1]]
            dX = ops.segment_pool_bwd(d_ptr, dev(env, G), op, arg=arg, n_rows=int(sp[-1]))
            assert np.array_equal(bits(host(dX)), bits(pool_bwd(segptr, np.ascontiguousarray(G), op, arg=argr)))


def test_arguments_are_checked_before_the_kernel_sees_a_pointer(env):
    ops, torch, capi = env["ops"], env["torch"], env["capi"]
    X = dev(env, values("sum", 8))
    n_seg = len(table()) - 1
    for bad in (X.double(), X[:, ::2], X.reshape(-1), X.to(torch.int32)):
        with pytest.raises(capi.GnnxError):
            ops.segment_pool(env["segptr"], bad, "sum")
    with pytest.raises(capi.GnnxError):
        ops.segment_pool(env["segptr"], X, "sum", out=torch.empty((n_seg, 9), dtype=torch.float32, device=env["dev"]))
    with pytest.raises(capi.GnnxError):
        ops.segment_pool(env["segptr"], X, "max", arg_out=torch.empty((n_seg, 8), dtype=torch.int64, device=env["dev"]))
    G = dev(env, pool_ref.grad_values()[0][:, :8])
    for bad in (G.double(), G[:-1], G.t().contiguous().t()):
        with pytest.raises(capi.GnnxError):
            ops.segment_pool_bwd(env["segptr"], bad, "sum", n_rows=X.shape[0])
    with pytest.raises(capi.GnnxError):
        ops.segment_pool_bwd(env["segptr"], G, "max", arg=None, n_rows=X.shape[0])
    with pytest.raises(capi.GnnxError):
        ops.segment_pool_bwd(env["segptr"], G, "sum", out=torch.empty((X.shape[0], 9), dtype=torch.float32, device=env["dev"]))
    # SUM and MEAN ignore the arg's leading dimension: they never touch it
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    Y = torch.empty((n_seg, 8), dtype=torch.float32, device=env["dev"])
    arg = torch.full((n_seg, 8), ARG_FILL, dtype=torch.int32, device=env["dev"])
    need = C.c_size_t(0)
    capi.call("gnnx_segment_pool_workspace", n_seg, X.shape[0], 8, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=env["dev"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = capi.lib()
    assert L.gnnx_segment_pool_f32(0, n_seg, X.shape[0], 8, p(env["segptr"]), p(X), 8, p(Y), 8, p(arg), 3, p(ws), need.value, stream) == 0
    assert L.gnnx_segment_pool_f32(2, n_seg, X.shape[0], 8, p(env["segptr"]), p(X), 8, p(Y), 8, p(arg), 3, p(ws), need.value, stream) == -1
    assert np.array_equal(bits(host(Y)), bits(pool_ref.reference("sum")[0][:, :8])) and bool((arg == ARG_FILL).all())


def test_max_backward_routes_each_gradient_to_the_forwards_arg(env):
    ops = env["ops"]
    F = 20
    sp = table().astype(np.int64)
    G = pool_ref.grad_values()[0][:, :F]
    assert (G != 0).all()
    Y, arg = ops.segment_pool(env["segptr"], dev(env, values("max", F)), "max")
    dX = host(ops.segment_pool_bwd(env["segptr"], dev(env, G), "max", arg=arg, n_rows=int(sp[-1])))
    arg = host(arg)
    for b in range(len(sp) - 1):
        rows = dX[sp[b]:sp[b + 1]]
        if len(rows) == 0:
            assert (arg[b] == -1).all()
            continue
        assert ((rows != 0).sum(axis=0) == 1).all(), b                               # exactly one row per (segment, feature)
        assert np.array_equal(sp[b] + np.argmax(rows != 0, axis=0), arg[b]), b       # and it is the forward's arg
        assert np.array_equal(bits(rows[arg[b] - sp[b], np.arange(F)]), bits(G[b])), b


def test_degenerate_sizes(env):
    ops, torch = env["ops"], env["torch"]
    d = env["dev"]
    nan = float("nan")
    X = dev(env, values("sum", 8))
    for op in pool_ref.OPS:
        # n_feat == 0: nothing to write
        Y, arg = ops.segment_pool(env["segptr"], X[:, :0], op)
        assert tuple(Y.shape) == (len(table()) - 1, 0)
        assert tuple(ops.segment_pool_bwd(env["segptr"], Y, op, arg=arg, n_rows=X.shape[0]).shape) == (X.shape[0], 0)
        # n_seg == 0
        ptr0 = dev(env, np.zeros(1, dtype=np.int32))
        Y, arg = ops.segment_pool(ptr0, X[:0], op)
        assert tuple(Y.shape) == (0, 8)
        assert tuple(ops.segment_pool_bwd(ptr0, Y, op, arg=arg, n_rows=0).shape) == (0, 8)
        # n_rows == 0 with segments: the per-segment outputs are still written
        ptr = dev(env, np.zeros(4, dtype=np.int32))
        Y = torch.full((3, 8), nan, dtype=torch.float32, device=d)
        arg = torch.full((3, 8), ARG_FILL, dtype=torch.int32, device=d)
        ops.segment_pool(ptr, X[:0], op, out=Y, arg_out=arg)
        assert (bits(host(Y)) == 0).all()
        assert (host(arg) == (-1 if op == "max" else ARG_FILL)).all()
        assert tuple(ops.segment_pool_bwd(ptr, Y, op, arg=arg, n_rows=0).shape) == (0, 8)


def test_a_small_workspace_is_refused_with_nothing_written(env):
    torch, capi = env["torch"], env["capi"]
    L = capi.lib()
    F, n_seg, n_rows = 8, len(table()) - 1, int(table()[-1])
    X = dev(env, values("max", F))
    need = C.c_size_t(0)
    capi.call("gnnx_segment_pool_workspace", n_seg, n_rows, F, C.byref(need))
    assert need.value == pool_ref.workspace_bytes(n_rows, F)
    ws = torch.full((need.value,), 0x5A, dtype=torch.uint8, device=env["dev"])
    Y = torch.full((n_seg, F), float("nan"), dtype=torch.float32, device=env["dev"])
    arg = torch.full((n_seg, F), ARG_FILL, dtype=torch.int32, device=env["dev"])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for wsp, nbytes in ((p(ws), need.value - 1), (None, need.value), (p(ws), 0)):
        st = L.gnnx_segment_pool_f32(2, n_seg, n_rows, F, p(env["segptr"]), p(X), F, p(Y), F, p(arg), F, wsp, nbytes, stream)
        assert st == -4, "GNNX_ERR_WORKSPACE expected"
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all()) and bool((arg == ARG_FILL).all()) and bool((ws == 0x5A).all())
    capi.call("gnnx_segment_pool_f32", 2, n_seg, n_rows, F, p(env["segptr"]), p(X), F, p(Y), F, p(arg), F, p(ws), need.value, stream)
    Yr, argr = pool_ref.reference("max")
    assert np.array_equal(bits(host(Y)), bits(Yr[:, :F])) and np.array_equal(host(arg), argr[:, :F])


def test_same_bits_on_two_consecutive_runs(env):
    ops = env["ops"]
    F = 132
    G = dev(env, pool_ref.grad_values()[0][:, :F])
    for op in pool_ref.OPS:
        X = dev(env, values(op, F))
        runs = []
        for _ in range(2):
            Y, arg = ops.segment_pool(env["segptr"], X, op)
            dX = ops.segment_pool_bwd(env["segptr"], G, op, arg=arg, n_rows=X.shape[0])
            runs.append((bits(host(Y)), None if arg is None else host(arg), bits(host(dX))))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2]), op
        assert arg is None or np.array_equal(runs[0][1], runs[1][1]), op
