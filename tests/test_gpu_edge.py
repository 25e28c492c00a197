"""GPU tests of the edge-feature aggregation (run with -m gpu on an MI355X): ops.spmm_edge / ops.spmm_edge_bwd / ops.csr_entry_edges
against tests/edge_ref.py, every assertion bit for bit, on the pattern of tests/test_gpu_reduce.py (n = 9000; rows of 2 S + 5, S and
S + 1 entries, hub columns, empty and one-entry rows).

Widths: the dispatch (gnnx_edge.hip shape_of) has the cells VEC in {4, 1} x G in {4, 8, 16, 32, 64} lanes per row x one or several
feature tiles.  16, 20, 64, 128, 256, 260 are the 16-byte cells G = 4 .. 64 and two tiles; 3, 6, 13, 30, 70 the scalar cells G = 4 .. 32
and two tiles; the misaligned F = 64 cases are the scalar G = 64 cell."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.edge_ref import spmm_edge_bwd_ref, spmm_edge_ref
from tests.helpers import synth
from tests.test_gpu_reduce import N, bits, dev, env, graph, host, pattern, placed, strided  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [(F, "small") for F in (3, 6, 13, 16, 20, 30, 64, 70, 128, 256, 260)] + [(F, "uniform") for F in (13, 64, 260)]
LAYOUTS = ("x_off", "e_off", "y_off", "g_off", "de_off", "odd_ldx", "odd_lde", "odd_ldy", "odd_ldg", "odd_ldde")   # one failing condition each
VALUES = np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def inputs(F, kind):
    """(X, E, G, y0, eidx) of a width, drawn once: E has nnz + 7 rows, eidx names nnz of them in random order."""
    rng = np.random.default_rng(3000 + F)
    ne = pattern()["nnz"] + 7
    if kind == "small":      # m == +-0 and exact ties in every row
        X, E = rng.choice(VALUES, size=(N, F)), rng.choice(VALUES, size=(ne, F))
    else:                    # a wrong association or a wrong segment cut changes bits
        X, E = synth.uniform_pm1(51, (N, F)), synth.uniform_pm1(52, (ne, F))
    return X, E, synth.uniform_pm1(53 + F, (N, F)), synth.uniform_pm1(54 + F, (N, F)), rng.permutation(ne)[:ne - 7].astype(np.int32)


def run(env, graph, F, kind, msg, use_eidx, layout="aligned", beta=0, with_x=True):
    ops, torch = env["ops"], env["torch"]
    X, E, G, y0, eidx = inputs(F, kind)
    X, eidx = (X if with_x else None), (eidx if use_eidx else None)
    rp, ci, what = graph["rowptr"], graph["colidx"], f"F={F} {kind} {msg} eidx={use_eidx} {layout} beta={beta} X={with_x}"

    def put(a, name):
        return placed(env, a, ld=F + 1 if layout == "odd_ld" + name else None, off=1 if layout == name + "_off" else 0)

    def fresh(rows, name):
        return strided(env, rows, F, torch.float32, float("nan"), ld=F + 1 if layout == "odd_ld" + name else None, off=1 if layout == name + "_off" else 0)

    d_X, d_E, d_G, d_eidx = (None if X is None else put(X, "x")), put(E, "e"), put(G, "g"), (None if eidx is None else dev(env, eidx))
    Y, Ybuf = fresh(N, "y")
    if beta:
        Y.copy_(dev(env, y0))
    ops.spmm_edge(graph["d_rowptr"], graph["d_colidx"], d_X, d_E, eidx=d_eidx, msg=msg, out=Y, beta=float(beta))
    got = host(Y)
    assert np.isfinite(got).all(), what                                  # beta = 0 never reads the NaN it overwrites
    assert np.array_equal(bits(got), bits(spmm_edge_ref(rp, ci, X, E, eidx, msg, y0 if beta else None))), what
    if layout == "odd_ldy":                                              # columns beyond F are not touched
        assert bool(torch.isnan(Ybuf.view(N, F + 1)[:, F]).all()), what
    dE, _ = fresh(E.shape[0], "de")
    ops.spmm_edge_bwd(graph["d_rowptr"], graph["d_colidx"], d_X, d_E, d_G, eidx=d_eidx, msg=msg, out=dE)
    fill = np.full(E.shape, np.nan, dtype=np.float32)                    # named rows: the reference; the 7 others keep the fill
    assert np.array_equal(bits(host(dE)), bits(spmm_edge_bwd_ref(rp, ci, X, E, G, eidx, msg, fill))), what
    if layout == "aligned" and not beta:                                 # dX: the forward on the transposed pattern through eidx[map_t]
        dE0 = spmm_edge_bwd_ref(rp, ci, X, E, G, eidx, msg)
        eidx_t = graph["map_t"] if eidx is None else eidx[graph["map_t"]]
        dX = ops.spmm_edge(graph["d_rowptr_t"], graph["d_colidx_t"], None, dev(env, dE0), eidx=dev(env, eidx_t), msg="add", n_cols=N)
        assert np.array_equal(bits(host(dX)), bits(spmm_edge_ref(graph["rowptr_t"], graph["colidx_t"], None, dE0, eidx_t, "add"))), what


@pytest.mark.parametrize("use_eidx", (False, True))
@pytest.mark.parametrize("msg", ("add", "relu"))
@pytest.mark.parametrize("F,kind", CASES)
def test_bits_forward_dE_and_dX(env, graph, F, kind, msg, use_eidx):
    run(env, graph, F, kind, msg, use_eidx)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bits_when_one_vec4_condition_fails(env, graph, layout):
    run(env, graph, 64, "small", "relu", True, layout)


@pytest.mark.parametrize("beta,with_x", ((1, True), (0, False), (1, False)))
def test_bits_with_beta_and_without_x(env, graph, beta, with_x):
    for msg in ("add", "relu"):
        run(env, graph, 20, "uniform", msg, True, beta=beta, with_x=with_x)


def test_entry_edges_last_duplicate_wins_self_loops_ignored_missing_raises(env):
    ops, capi = env["ops"], env["capi"]
    src = np.array([0, 2, 0, 1, 3, 0, 2, 1], dtype=np.int32)            # (0, 1) three times, (1, 1) a self loop
    dst = np.array([1, 0, 1, 1, 2, 1, 3, 0], dtype=np.int32)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), 4)
    pairs = list(zip(np.repeat(np.arange(4), np.diff(host(g.rowptr))), host(g.colidx)))
    assert pairs == [(0, 1), (1, 0), (2, 0), (2, 3), (3, 2)]
    eidx = host(ops.csr_entry_edges(g.rowptr, g.colidx, dev(env, src), dev(env, dst)))
    assert eidx.tolist() == [5, 7, 1, 6, 4]
    with pytest.raises(capi.GnnxError, match="1 edges"):               # (3, 0) is not stored; neither endpoint order helps
        ops.csr_entry_edges(g.rowptr, g.colidx, dev(env, np.append(src, 3).astype(np.int32)), dev(env, np.append(dst, 0).astype(np.int32)))
    with pytest.raises(capi.GnnxError, match="1 edges"):               # a row outside the pattern
        ops.csr_entry_edges(g.rowptr, g.colidx, dev(env, np.append(src, 9).astype(np.int32)), dev(env, np.append(dst, 0).astype(np.int32)))
    with pytest.raises(ValueError, match="1 stored entries"):          # (3, 2) gets no edge
        ops.csr_entry_edges(g.rowptr, g.colidx, dev(env, np.delete(src, 4)), dev(env, np.delete(dst, 4)))


def test_statuses_and_workspace_bound(env, graph):
    """Bad arguments are GNNX_ERR_INVALID_ARG and one byte less than the (reductions') query GNNX_ERR_WORKSPACE, each with the outputs untouched; a
    workspace 4 bytes off gives the same bits."""
    torch, capi = env["torch"], env["capi"]
    L, F, nnz = capi.lib(), 64, graph["nnz"]
    X, E, G, _, _ = inputs(F, "small")
    d_X, d_E, d_G = dev(env, X), dev(env, E), dev(env, G)
    need = C.c_size_t(0)
    capi.call("gnnx_spmm_csr_reduce_workspace", N, nnz, F, C.byref(need))
    assert need.value > 3 * F * 4                                        # the hub row's partials are in it
    ws = torch.zeros(need.value + 4, dtype=torch.uint8, device=env["dev"])
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Y = torch.full((N, F), 7.0, dtype=torch.float32, device=env["dev"])
    dE = torch.full(E.shape, 7.0, dtype=torch.float32, device=env["dev"])

    def fwd(off=0, nbytes=need.value, msg=1, beta=0.0, ldx=F, ne=E.shape[0], nz=nnz):
        return L.gnnx_spmm_csr_edge_f32(N, N, F, nz, ptr(graph["d_rowptr"]), ptr(graph["d_colidx"]), None, ne, ptr(d_X), ldx, ptr(d_E), F, msg, beta,
                                        ptr(Y), F, ptr(ws, off), nbytes, stream)

    def bwd(off=0, nbytes=need.value, msg=1, ldg=F, ne=E.shape[0], nz=nnz):
        return L.gnnx_spmm_csr_edge_bwd_f32(N, N, F, nz, ptr(graph["d_rowptr"]), ptr(graph["d_colidx"]), None, ne, ptr(d_X), F, ptr(d_E), F, msg,
                                            ptr(d_G), ldg, ptr(dE), F, ptr(ws, off), nbytes, stream)

    bad = [fwd(msg=2), fwd(beta=0.5), fwd(ldx=F - 1), fwd(ne=nnz - 1), fwd(nz=2 ** 31), fwd(nz=-1),
           bwd(msg=-1), bwd(ldg=F - 1), bwd(ne=nnz - 1), bwd(nz=2 ** 31)]
    assert bad == [-1] * len(bad)
    assert fwd(nbytes=need.value - 1) == -4 and bwd(off=4, nbytes=need.value - 1) == -4
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all()) and bool((dE == 7.0).all())
    Yr, dEr = spmm_edge_ref(graph["rowptr"], graph["colidx"], X, E), spmm_edge_bwd_ref(graph["rowptr"], graph["colidx"], X, E, G, fill=host(dE))
    for off in (0, 4):
        assert fwd(off) == 0 and bwd(off) == 0
        assert np.array_equal(bits(host(Y)), bits(Yr)) and np.array_equal(bits(host(dE)), bits(dEr))
