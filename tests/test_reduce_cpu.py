"""CPU checks of the neighbourhood reductions' restatement (tests/reduce_ref.py) and of the C-ABI's argument validation: the forward
against a plain double loop on a graph full of ties, signed zeros, -inf, empty and one-entry rows; the backward's segment order (with
S = 4 so that small rows have several segments) against the same sums as explicit loops; exact routing (every (row, feature) of a
non-empty row reaches exactly one entry); float64 autograd; and tests/spmm_ref.py on the transposed pattern for rows of one segment."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests.helpers import ROOT, pkg  # noqa: F401
from tests.reduce_ref import spmm_reduce_bwd_ref, spmm_reduce_ref, transpose_csr
from tests.spmm_ref import spmm_ref

N, F = 40, 5


def small_graph(seed=7):
    """40 vertices: rows 3, 11, 29 empty, row 5 one entry, row 0 with 23 entries, the rest 0 .. 9; ascending columns, no duplicates."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(N):
        d = {0: 23, 3: 0, 11: 0, 29: 0, 5: 1}.get(i, int(rng.integers(0, 10)))
        rows.append(np.sort(rng.choice(N, size=d, replace=False)))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colidx = np.concatenate(rows).astype(np.int32)
    return rowptr, colidx


@pytest.fixture(scope="module")
def graph():
    rowptr, colidx = small_graph()
    deg = np.diff(rowptr)
    assert (deg == 0).sum() >= 3 and (deg == 1).any() and deg.max() == 23
    rowptr_t, colidx_t, map_t = transpose_csr(rowptr, colidx, N)
    assert np.diff(rowptr_t).max() > 8      # several segments of S = 4
    rng = np.random.default_rng(11)
    X = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2, -np.inf], dtype=np.float32), size=(N, F))
    X[colidx[rowptr[7]:rowptr[8]]] = -np.inf          # a whole neighbourhood of -inf (if row 7 has entries)
    vals = rng.choice(np.array([-1, 0.5, 1], dtype=np.float32), size=len(colidx))
    return dict(rowptr=rowptr, colidx=colidx, rowptr_t=rowptr_t, colidx_t=colidx_t, map_t=map_t, X=X, vals=vals)


def loop_forward(rowptr, colidx, X, vals, op):
    better = (lambda a, b: a > b) if op == "max" else (lambda a, b: a < b)
    Y = np.zeros((len(rowptr) - 1, X.shape[1]), dtype=np.float32)
    arg = np.full(Y.shape, -1, dtype=np.int32)
    for i in range(len(rowptr) - 1):
        for f in range(X.shape[1]):
            for p in range(rowptr[i], rowptr[i + 1]):
                t = X[colidx[p], f] if vals is None else np.float32(vals[p] * X[colidx[p], f])
                if arg[i, f] < 0 or better(t, Y[i, f]):
                    Y[i, f], arg[i, f] = t, p
    return Y, arg


@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("with_vals", [False, True])
def test_forward_restatement_vs_double_loop(graph, op, with_vals):
    vals = graph["vals"] if with_vals else None
    with np.errstate(invalid="ignore"):
        Y, arg = spmm_reduce_ref(graph["rowptr"], graph["colidx"], graph["X"], vals, op)
        Yl, argl = loop_forward(graph["rowptr"], graph["colidx"], graph["X"], vals, op)
    assert np.array_equal(arg, argl)
    assert np.array_equal(Y.view(np.int32), Yl.view(np.int32))     # bits: the sign of a winning zero
    deg = np.diff(graph["rowptr"])
    assert (arg[deg == 0] == -1).all() and (Y[deg == 0].view(np.int32) == 0).all()
    assert (arg[deg > 0] >= graph["rowptr"][:-1][deg > 0, None]).all() and (arg[deg > 0] < graph["rowptr"][1:][deg > 0, None]).all()
    if not with_vals:                                              # ties and signed zeros did occur
        T = graph["X"][graph["colidx"]]
        assert any((T[b:e] == Y[i]).sum(0).max() > 1 for i, (b, e) in enumerate(zip(graph["rowptr"][:-1], graph["rowptr"][1:])) if e > b)
        assert (Y.view(np.int32) == np.float32(-0.0).view(np.int32)).any()


def finite_inputs(graph, seed=13):
    rng = np.random.default_rng(seed)
    X = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32), size=(N, F))
    G = rng.uniform(-1, 1, size=(N, F)).astype(np.float32)
    return X, G


@pytest.mark.parametrize("with_vals", [False, True])
@pytest.mark.parametrize("beta", [0, 1])
def test_backward_restatement_vs_explicit_loops(graph, with_vals, beta):
    S = 4
    X, G = finite_inputs(graph)
    vals = graph["vals"] if with_vals else None
    _, arg = spmm_reduce_ref(graph["rowptr"], graph["colidx"], X, vals, "max")
    y0 = np.random.default_rng(5).uniform(-1, 1, size=(N, F)).astype(np.float32) if beta else None
    got = spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], arg, G, vals, y0, S=S)
    rp, ci, mp = graph["rowptr_t"], graph["colidx_t"], graph["map_t"]
    ref = np.zeros((N, F), dtype=np.float32)
    for c in range(N):
        for f in range(F):
            row = None
            for b in range(rp[c], rp[c + 1], S):
                acc = np.float32(0)
                for q in range(min(b + S, rp[c + 1]) - 1, b - 1, -1):
                    if arg[ci[q], f] == mp[q]:
                        t = G[ci[q], f] if vals is None else np.float32(vals[mp[q]] * G[ci[q], f])
                        acc = np.float32(acc + t)
                row = acc if row is None else np.float32(row + acc)
            row = np.float32(0) if row is None else row
            ref[c, f] = row if y0 is None else np.float32(y0[c, f] + row)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    if not beta:   # S matters: the one-segment order differs somewhere on this graph
        assert not np.array_equal(got, spmm_reduce_bwd_ref(rp, ci, mp, arg, G, vals, y0))


@pytest.mark.parametrize("op", ["max", "min"])
def test_every_gradient_element_is_routed_exactly_once(graph, op):
    X, _ = finite_inputs(graph)
    G = np.random.default_rng(3).integers(-8, 9, size=(N, F)).astype(np.float32)
    _, arg = spmm_reduce_ref(graph["rowptr"], graph["colidx"], X, None, op)
    for S in (4, 4096):
        dX = spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], arg, G, None, None, S=S)
        assert np.array_equal(dX.sum(0), G[np.diff(graph["rowptr"]) > 0].sum(0))


def test_backward_vs_float64_autograd_without_ties(graph):
    import torch
    rng = np.random.default_rng(17)
    X = rng.uniform(-1, 1, size=(N, F)).astype(np.float32)
    vals = rng.choice(np.array([0.5, 1, 2], dtype=np.float32), size=len(graph["colidx"]))      # exact products in either precision
    G = rng.uniform(-1, 1, size=(N, F)).astype(np.float32)
    rowptr, colidx = graph["rowptr"], graph["colidx"]
    T = vals[:, None] * X[colidx]
    for b, e in zip(rowptr[:-1], rowptr[1:]):
        if e - b > 1:
            top = np.sort(T[b:e], axis=0)
            assert (top[-1] > top[-2]).all()                       # no ties
    Y, arg = spmm_reduce_ref(rowptr, colidx, X, vals, "max")
    got = spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], arg, G, vals)
    rows_e = torch.from_numpy(np.repeat(np.arange(N), np.diff(rowptr)))
    X64 = torch.tensor(X.astype(np.float64), requires_grad=True)
    T64 = torch.from_numpy(vals.astype(np.float64))[:, None] * X64[torch.from_numpy(colidx.astype(np.int64))]
    Y64 = torch.zeros((N, F), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, F), T64, "amax", include_self=False)
    assert np.array_equal(Y64.detach().numpy(), Y.astype(np.float64))
    (Y64 * torch.from_numpy(G.astype(np.float64))).sum().backward()
    ref = X64.grad.numpy()
    # float32 rounding of the sums: each of the k <= d routed terms is exact here (vals a power of two), each add rounds once
    hit = arg[np.repeat(np.arange(N), np.diff(rowptr))] == np.arange(len(colidx))[:, None]
    absum = np.zeros((N, F))
    np.add.at(absum, colidx, np.abs(vals[:, None].astype(np.float64) * G[rows_e.numpy()]) * hit)
    bound = np.diff(graph["rowptr_t"]).max() * 2.0 ** -24 * absum
    assert (np.abs(got - ref) <= bound).all()
    assert np.abs(ref).max() > 0


def test_backward_of_one_segment_rows_is_the_aggregation_on_the_transposed_pattern(graph):
    """For rows of at most S entries the routed sum is spmm_ref on CSR(A^T) with the 0/1 match folded into the values, a column at a time."""
    X, G = finite_inputs(graph)
    for vals in (None, graph["vals"]):
        _, arg = spmm_reduce_ref(graph["rowptr"], graph["colidx"], X, vals, "max")
        got = spmm_reduce_bwd_ref(graph["rowptr_t"], graph["colidx_t"], graph["map_t"], arg, G, vals)
        for f in range(F):
            match = (arg[graph["colidx_t"], f] == graph["map_t"]).astype(np.float32)
            v = match if vals is None else vals[graph["map_t"]] * match
            col = spmm_ref(graph["rowptr_t"], graph["colidx_t"], G[:, f:f + 1], vals=v)
            assert np.array_equal(got[:, f:f + 1], col)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_argument_validation_without_device(capi):
    """Validation happens before any HIP call, so these return statuses even with no GPU."""
    L = capi.lib()
    INVALID, WORKSPACE = -1, -4
    b = C.c_size_t(0)
    assert L.gnnx_spmm_csr_reduce_workspace(1000, 5000, 64, C.byref(b)) == 0 and b.value >= 512
    small = b.value
    assert L.gnnx_spmm_csr_reduce_workspace(1000, 10_000_000, 64, C.byref(b)) == 0 and b.value > small
    hubs, segs = min(10_000_000 // 4097, 1000), 10_000_000 // 4096 + min(10_000_000 // 4097, 1000)
    assert b.value == 256 + -(-4 * (16 + 2 * hubs + segs + 2 * segs * 64) // 256) * 256          # the header's formula
    assert L.gnnx_spmm_csr_reduce_workspace(1000, 5000, 64, None) == INVALID
    assert L.gnnx_spmm_csr_reduce_workspace(-1, 5000, 64, C.byref(b)) == INVALID
    assert L.gnnx_spmm_csr_reduce_workspace(1000, 1 << 31, 64, C.byref(b)) == INVALID
    p = C.c_void_p(4096)    # never dereferenced: every call below fails before a device is touched

    def fwd(op=0, n_rows=4, n_cols=4, F=8, nnz=6, rowptr=p, colidx=p, vals=None, X=p, ldx=8, Y=p, ldy=8, arg=p, lda=8, ws=p, wsb=1 << 20):
        return L.gnnx_spmm_csr_reduce_f32(op, n_rows, n_cols, F, nnz, rowptr, colidx, vals, X, ldx, Y, ldy, arg, lda, ws, wsb, None)

    def bwd(n_rows=4, n_cols=4, F=8, nnz=6, rowptr=p, colidx=p, map_t=p, vals=None, arg=p, lda=8, G=p, ldg=8, beta=0.0, dX=p, ldx=8, ws=p,
            wsb=1 << 20):
        return L.gnnx_spmm_csr_reduce_bwd_f32(n_rows, n_cols, F, nnz, rowptr, colidx, map_t, vals, arg, lda, G, ldg, beta, dX, ldx, ws, wsb, None)

    for k in ("rowptr", "colidx", "X", "Y"):
        assert fwd(**{k: None}) == INVALID, k
        assert b"null" in L.gnnx_last_error()
    for k in ("rowptr", "colidx", "map_t", "arg", "G", "dX"):
        assert bwd(**{k: None}) == INVALID, k
    for k in ("n_rows", "n_cols", "F", "nnz"):
        assert fwd(**{k: -1}) == INVALID and bwd(**{k: -1}) == INVALID, k
    assert fwd(nnz=1 << 31) == INVALID and bwd(nnz=1 << 31) == INVALID
    for k in ("ldx", "ldy", "lda"):
        assert fwd(**{k: 7}) == INVALID, k
    for k in ("lda", "ldg", "ldx"):
        assert bwd(**{k: 7}) == INVALID, k
    assert fwd(op=2) == INVALID and fwd(op=-1) == INVALID
    assert bwd(beta=0.5) == INVALID and bwd(beta=2.0) == INVALID
    assert fwd(ws=None) == WORKSPACE and bwd(ws=None) == WORKSPACE
    assert fwd(wsb=16) == WORKSPACE and bwd(wsb=16) == WORKSPACE
    assert fwd(n_rows=0) == 0 and fwd(F=0, ldx=0, ldy=0, lda=0) == 0           # nothing to write: no device call either
    assert bwd(n_rows=0) == 0 and bwd(F=0, ldx=0, ldg=0, lda=0) == 0
