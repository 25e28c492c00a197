"""GPU tests of the neighbourhood reductions (run with -m gpu on an MI355X): ops.spmm_reduce / ops.spmm_reduce_bwd against
tests/reduce_ref.py, bit for bit in value and arg.

The pattern is a square n = 9000 graph with rows and columns on both sides of the segment length S = 4096 (a hub row of 2 S + 5
entries, rows of exactly S and S + 1, a hub column of 2 S + 5 and a column of exactly S), empty rows and one-entry rows.

Widths.  The dispatch (gnnx_reduce.hip shape_of) has the cells VEC in {4, 1} x G in {4, 8, 16, 32, 64} lanes per row x one or several
feature tiles.  The issue's forward list (1, 3, 4, 6, 16, 20, 36, 64, 68, 128, 132, 256, 260, 516) covers every 16-byte cell and the
scalar cells G = 4 and 8; it misses the scalar cells G = 16 (9 .. 16 features), G = 32 (17 .. 32) and the scalar kernel on several
tiles (more than 64 features): 13, 30 and 70 are added for those (the misaligned F = 64 cases are the scalar G = 64 cell).  The
issue's backward list (1, 5, 16, 64, 132, 256) is extended by the same three and by 20, 128 and 260 (16-byte cells G = 8, G = 32 and
two tiles)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from tests.helpers import synth
from tests.reduce_ref import SEG, spmm_reduce_bwd_ref, spmm_reduce_ref, transpose_csr
from tests.spmm_ref import spmm_ref

pytestmark = pytest.mark.gpu

N = 9000
S = SEG
FWD_WIDTHS = (1, 3, 4, 6, 13, 16, 20, 30, 36, 64, 68, 70, 128, 132, 256, 260, 516)
BWD_WIDTHS = (1, 5, 13, 16, 20, 30, 64, 70, 128, 132, 256, 260)
FWD_LAYOUTS = ("x_off", "odd_ldx", "odd_ldy", "odd_lda", "arg_off")       # one failing vec4 condition each, at F = 64
BWD_LAYOUTS = ("g_off", "odd_ldg", "odd_lda", "odd_ldx", "arg_off")
X_VALUES = np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32)
V_VALUES = np.array([-1, 0.5, 1], dtype=np.float32)


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def pattern():
    """Rows 0 / 1 / 2 and columns 3 / 4 carry the long runs; rows 100 .. 124 are empty, rows 200 .. 224 have one entry; the special
    rows use columns >= 5 only and the columns 3 and 4 sit in rows >= 300 only, so the counts are exact."""
    rng = np.random.default_rng(2024)
    A = np.zeros((N, N), dtype=bool)
    A[rng.integers(300, N, 4 * N), rng.integers(5, N, 4 * N)] = True
    for row, d in ((0, 2 * S + 5), (1, S), (2, S + 1)):
        A[row, 5 + rng.choice(N - 5, d, replace=False)] = True
    for row in range(200, 225):
        A[row, rng.integers(5, N)] = True
    A[300 + rng.choice(N - 300, 2 * S + 5, replace=False), 3] = True
    A[300 + rng.choice(N - 300, S, replace=False), 4] = True
    rows, cols = np.nonzero(A)                       # row-major: ascending columns, no duplicates
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int32)
    colidx = cols.astype(np.int32)
    rowptr_t, colidx_t, map_t = transpose_csr(rowptr, colidx, N)
    deg, deg_t = np.diff(rowptr), np.diff(rowptr_t)
    assert (deg == 0).sum() >= 20 and (deg == 1).sum() >= 20
    assert deg[0] == 2 * S + 5 and deg[1] == S and deg[2] == S + 1
    assert deg_t[3] == 2 * S + 5 and deg_t[4] == S
    assert 3.5 <= np.median(deg[300:]) <= 8
    for b, e in zip(rowptr[:3], rowptr[1:4]):
        assert (np.diff(colidx[b:e]) > 0).all()
    return dict(rowptr=rowptr, colidx=colidx, rowptr_t=rowptr_t, colidx_t=colidx_t, map_t=map_t, nnz=len(colidx))


@pytest.fixture(scope="module")
def graph(env):
    p = dict(pattern())
    for k in ("rowptr", "colidx", "rowptr_t", "colidx_t"):
        p["d_" + k] = dev(env, p[k])
    p["d_map_t"] = env["ops"].csr_transpose_map(p["d_rowptr"], p["d_colidx"], p["d_rowptr_t"], p["d_colidx_t"])
    assert np.array_equal(host(p["d_map_t"]), p["map_t"])
    return p


@functools.lru_cache(maxsize=None)
def inputs(F, kind="small"):
    """(X, vals, G, y0) of a width, drawn once."""
    rng = np.random.default_rng(1000 + F)
    nnz = pattern()["nnz"]
    if kind == "small":      # ties and signed zeros everywhere
        X, vals = rng.choice(X_VALUES, size=(N, F)), rng.choice(V_VALUES, size=nnz)
    else:
        X, vals = synth.uniform_pm1(31, (N, F)), synth.uniform_pm1(32, (nnz,))
    return X, vals, synth.uniform_pm1(33 + F, (N, F)), synth.uniform_pm1(34 + F, (N, F))


@functools.lru_cache(maxsize=None)
def forward_ref(F, kind, with_vals, op):
    p = pattern()
    X, vals, _, _ = inputs(F, kind)
    return spmm_reduce_ref(p["rowptr"], p["colidx"], X, vals if with_vals else None, op)


def strided(env, rows, F, dtype, fill, ld=None, off=0):
    """A [rows, F] view on a leading dimension ld, `off` elements into its buffer, every element (pad columns too) set to `fill`."""
    torch = env["torch"]
    ld = F if ld is None else ld
    buf = torch.full((rows * ld + off,), fill, dtype=dtype, device=env["dev"])
    return buf[off:].view(rows, ld)[:, :F], buf


def placed(env, a, ld=None, off=0):
    view, _ = strided(env, a.shape[0], a.shape[1], env["torch"].from_numpy(a[:1]).dtype, 0, ld, off)
    view.copy_(dev(env, a))
    return view


def run_forward(env, graph, F, kind, layout):
    ops, torch = env["ops"], env["torch"]
    X, vals, _, _ = inputs(F, kind)
    d_X = placed(env, X, ld=F + 1 if layout == "odd_ldx" else None, off=1 if layout == "x_off" else 0)
    d_vals = dev(env, vals)
    for op in ("max", "min"):
        for with_vals in (False, True):
            Y, Ybuf = strided(env, N, F, torch.float32, float("nan"), ld=F + 1 if layout == "odd_ldy" else None)
            arg, argbuf = strided(env, N, F, torch.int32, -7, ld=F + 1 if layout == "odd_lda" else None, off=1 if layout == "arg_off" else 0)
            ops.spmm_reduce(graph["d_rowptr"], graph["d_colidx"], d_X, op=op, vals=d_vals if with_vals else None, out=Y, arg_out=arg)
            Yr, argr = forward_ref(F, kind, with_vals, op)
            what = f"F={F} {layout} {op} vals={with_vals}"
            assert np.array_equal(host(arg), argr), what
            assert np.array_equal(bits(host(Y)), bits(Yr)), what
            if layout == "odd_ldy":     # columns beyond F are not touched
                assert bool(torch.isnan(Ybuf.view(N, F + 1)[:, F]).all()), what
            if layout == "odd_lda":
                assert bool((argbuf.view(N, F + 1)[:, F] == -7).all()), what
            if not with_vals and op == "max":   # without the arg: the same values
                Y2, none = ops.spmm_reduce(graph["d_rowptr"], graph["d_colidx"], d_X, op=op, want_arg=False)
                assert none is None and np.array_equal(bits(host(Y2)), bits(Yr)), what


@pytest.mark.parametrize("F", FWD_WIDTHS)
def test_forward_bits_value_and_arg(env, graph, F):
    run_forward(env, graph, F, "small", "aligned")


@pytest.mark.parametrize("layout", FWD_LAYOUTS)
def test_forward_bits_when_one_vec4_condition_fails(env, graph, layout):
    run_forward(env, graph, 64, "small", layout)


def test_forward_bits_uniform_values(env, graph):
    run_forward(env, graph, 32, "uniform", "aligned")


def test_ties_across_segments_go_to_the_first_entry(env, graph):
    """Every row of X equal: every entry of a row ties, in every segment; a combine that prefers a later segment fails here."""
    ops = env["ops"]
    F = 64
    X = np.broadcast_to(np.random.default_rng(5).choice(X_VALUES, size=(1, F)), (N, F)).copy()
    for op in ("max", "min"):
        Y, arg = ops.spmm_reduce(graph["d_rowptr"], graph["d_colidx"], dev(env, X), op=op)
        Yr, argr = spmm_reduce_ref(graph["rowptr"], graph["colidx"], X, None, op)
        assert (host(arg)[0] == graph["rowptr"][0]).all() and (host(arg)[2] == graph["rowptr"][2]).all()
        assert np.array_equal(host(arg), argr) and np.array_equal(bits(host(Y)), bits(Yr))


@pytest.mark.parametrize("op,inf", [("max", -np.inf), ("min", np.inf)])
def test_a_neighbourhood_of_infinities_still_gets_its_first_entry(env, graph, op, inf):
    ops = env["ops"]
    F = 20
    rp, ci = graph["rowptr"], graph["colidx"]
    short = 300 + int(np.argmax(np.diff(rp)[300:] == 3))
    assert rp[short + 1] - rp[short] == 3
    X = inputs(F)[0].copy()
    for row in (0, short):
        X[ci[rp[row]:rp[row + 1]]] = inf
    Y, arg = ops.spmm_reduce(graph["d_rowptr"], graph["d_colidx"], dev(env, X), op=op)
    Y, arg = host(Y), host(arg)
    for row in (0, short):
        assert (Y[row] == inf).all() and (arg[row] == rp[row]).all()
    Yr, argr = spmm_reduce_ref(rp, ci, X, None, op)
    assert np.array_equal(arg, argr) and np.array_equal(bits(Y), bits(Yr))


def run_backward(env, graph, F, layout):
    ops, torch = env["ops"], env["torch"]
    _, vals, G, y0 = inputs(F)
    d_G = placed(env, G, ld=F + 1 if layout == "odd_ldg" else None, off=1 if layout == "g_off" else 0)
    d_vals = dev(env, vals)
    for with_vals in (False, True):
        _, arg = forward_ref(F, "small", with_vals, "max")
        d_arg = placed(env, arg, ld=F + 1 if layout == "odd_lda" else None, off=1 if layout == "arg_off" else 0)
        v = vals if with_vals else None
        for beta in (0, 1):
            dX, buf = strided(env, N, F, torch.float32, float("nan"), ld=F + 1 if layout == "odd_ldx" else None)
            if beta:
                dX.copy_(dev(env, y0))
            ops.spmm_reduce_bwd(graph["d_rowptr_t"], graph["d_colidx_t"], graph["d_map_t"], d_arg, d_G, vals=d_vals if with_vals else None,
                                out=dX, beta=float(beta))
            ref = spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], arg, G, v, y0 if beta else None)
            what = f"F={F} {layout} vals={with_vals} beta={beta}"
            got = host(dX)
            assert np.isfinite(got).all(), what            # beta = 0 never reads the NaN it overwrites
            assert np.array_equal(bits(got), bits(ref)), what
            if layout == "odd_ldx":
                assert bool(torch.isnan(buf.view(N, F + 1)[:, F]).all()), what


@pytest.mark.parametrize("F", BWD_WIDTHS)
def test_backward_bits(env, graph, F):
    run_backward(env, graph, F, "aligned")


@pytest.mark.parametrize("layout", BWD_LAYOUTS)
def test_backward_bits_when_one_vec4_condition_fails(env, graph, layout):
    run_backward(env, graph, 64, layout)


def test_one_entry_rows_are_the_aggregation(env):
    """Every row has exactly one entry: the forward is spmm(vals) and the backward spmm on the transposed pattern with vals[map_t], bit for
    bit (values without zeros: the sum's +0 start would turn a -0 product into +0)."""
    ops = env["ops"]
    n, F = 5000, 36
    cols = np.random.default_rng(9).integers(0, n, n).astype(np.int32)
    rowptr = np.arange(n + 1, dtype=np.int32)
    rowptr_t, colidx_t, map_np = transpose_csr(rowptr, cols, n)
    assert np.diff(rowptr_t).max() > 2
    d = {k: dev(env, v) for k, v in dict(rp=rowptr, ci=cols, rpt=rowptr_t, cit=colidx_t).items()}
    map_t = ops.csr_transpose_map(d["rp"], d["ci"], d["rpt"], d["cit"])
    X, vals, G = (dev(env, synth.uniform_pm1(s, shape)) for s, shape in ((41, (n, F)), (42, (n,)), (43, (n, F))))
    for v in (None, vals):
        for op in ("max", "min"):
            Y, arg = ops.spmm_reduce(d["rp"], d["ci"], X, op=op, vals=v)
            assert env["torch"].equal(Y, ops.spmm(d["rp"], d["ci"], X, vals=v))
            assert np.array_equal(host(arg), np.broadcast_to(np.arange(n, dtype=np.int32)[:, None], (n, F)))
        dX = ops.spmm_reduce_bwd(d["rpt"], d["cit"], map_t, arg, G, vals=v)
        assert env["torch"].equal(dX, ops.spmm(d["rpt"], d["cit"], G, vals=None if v is None else v[map_t.long()].contiguous()))


def test_workspace_bound_and_placement(env, graph):
    """One byte less than the query is GNNX_ERR_WORKSPACE with the outputs untouched; a workspace 4 bytes off gives the same bits."""
    torch, capi, ops = env["torch"], env["capi"], env["ops"]
    L = capi.lib()
    F, nnz = 64, graph["nnz"]
    X, vals, G, _ = inputs(F)
    d_X, d_G = dev(env, X), dev(env, G)
    Yr, argr = forward_ref(F, "small", False, "max")
    d_argr = dev(env, argr)
    need = C.c_size_t(0)
    capi.call("gnnx_spmm_csr_reduce_workspace", N, nnz, F, C.byref(need))
    assert need.value > 2 * 3 * F * 4            # the hub rows' partials are in it
    ws = torch.zeros(need.value + 4, dtype=torch.uint8, device=env["dev"])
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(Y, arg, off, nbytes):
        return L.gnnx_spmm_csr_reduce_f32(0, N, N, F, nnz, ptr(graph["d_rowptr"]), ptr(graph["d_colidx"]), None, ptr(d_X), F, ptr(Y), F, ptr(arg), F,
                                          ptr(ws, off), nbytes, stream)

    def bwd(dX, off, nbytes):
        return L.gnnx_spmm_csr_reduce_bwd_f32(N, N, F, nnz, ptr(graph["d_rowptr_t"]), ptr(graph["d_colidx_t"]), ptr(graph["d_map_t"]), None,
                                              ptr(d_argr), F, ptr(d_G), F, 0.0, ptr(dX), F, ptr(ws, off), nbytes, stream)

    dXr = spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], argr, G)
    for off in (0, 4):
        Y = torch.full((N, F), 7.0, dtype=torch.float32, device=env["dev"])
        arg = torch.full((N, F), -7, dtype=torch.int32, device=env["dev"])
        dX = torch.full((N, F), 7.0, dtype=torch.float32, device=env["dev"])
        assert fwd(Y, arg, off, need.value - 1) == -4 and bwd(dX, off, need.value - 1) == -4
        torch.cuda.synchronize()
        assert bool((Y == 7.0).all()) and bool((arg == -7).all()) and bool((dX == 7.0).all())
        assert fwd(Y, arg, off, need.value) == 0 and bwd(dX, off, need.value) == 0
        assert np.array_equal(bits(host(Y)), bits(Yr)) and np.array_equal(host(arg), argr)
        assert np.array_equal(bits(host(dX)), bits(dXr))


def test_two_runs_give_the_same_bits(env, graph):
    ops, torch = env["ops"], env["torch"]
    F = 64
    X, vals, G, _ = inputs(F, "uniform")
    d_X, d_vals, d_G = dev(env, X), dev(env, vals), dev(env, G)
    runs = []
    for _ in range(2):
        Y, arg = ops.spmm_reduce(graph["d_rowptr"], graph["d_colidx"], d_X, vals=d_vals)
        dX = ops.spmm_reduce_bwd(graph["d_rowptr_t"], graph["d_colidx_t"], graph["d_map_t"], arg, d_G, vals=d_vals)
        runs.append((Y.clone(), arg.clone(), dX.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert np.array_equal(bits(host(runs[0][2])),
                          bits(spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], host(runs[0][1]), G, vals)))
