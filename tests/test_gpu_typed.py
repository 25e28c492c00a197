"""GPU tests of the relation-typed aggregation (run with -m gpu on an MI355X): ops.spmm_typed, ops.spmm_typed_bwd on the transposed
pattern and ops.typed_coeff_grad against tests/typed_ref.py, bit for bit, on the pattern of tests/test_gpu_reduce.py (n = 9000; rows of
2 S + 5, S and S + 1 entries, hub columns, empty and one-entry rows).  The types are drawn per entry from a fixed seed among the first
R - 1 relations: the last one never occurs and its slab must be +0.

Cases (F, R, B or None for one-hot, vals): F = 3 scalar lanes, 16 / 20 / 64 the vector groups of 4 / 8 / 16 lanes, 260 two feature
tiles; one-hot R = 3 is a partial register tile, R = 11 two slab tiles with the second partial, bases (5, 2) and (40, 8) full tiles,
(7, 9) two tiles in basis mode.  The exact leg reruns the F = 20 cases on small integers and halves, where every sum is exact in float32
in any order, against a float64 evaluation over the COO form: it holds the restatement and the kernels to an independent reference."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.helpers import synth
from tests.test_gpu_reduce import N, bits, dev, env, graph, host, pattern, placed, strided  # noqa: F401
from tests.typed_ref import spmm_typed_bwd_ref, spmm_typed_ref, typed_coeff_grad_ref

pytestmark = pytest.mark.gpu

MODES = ((3, None), (11, None), (5, 2), (40, 8), (7, 9))
CASES = [(F, R, B, True) for F in (20, 64) for R, B in MODES] + [(F, R, B, True) for F in (3, 16, 260) for R, B in (MODES[0], MODES[2])] + \
        [(20, 3, None, False), (20, 5, 2, False)]


@functools.lru_cache(maxsize=None)
def data(F, R, B, with_vals, kind="uniform"):
    """Host inputs of a case and the three reference results, computed once."""
    p, rng = pattern(), np.random.default_rng(7 * F + R)
    nnz, width = p["nnz"], (R if B is None else B) * F
    etype = rng.integers(0, R - 1, nnz).astype(np.int32)
    if kind == "uniform":
        X, dM, vals = synth.uniform_pm1(41 + F, (N, F)), synth.uniform_pm1(42 + F, (N, width)), synth.uniform_pm1(43, (nnz,))
        coeff = None if B is None else synth.uniform_pm1(44 + R, (R, B))
    else:
        pick = lambda values, shape: rng.choice(np.array(values, dtype=np.float32), size=shape)  # noqa: E731
        X, dM, vals = pick([-2, -1, 0, 1, 2], (N, F)), pick([-2, -1, 0, 1, 2], (N, width)), pick([0.5, 1, 2], nnz)
        coeff = None if B is None else pick([-1, 0, 1, 2], (R, B))
    vals = vals if with_vals else None
    d = dict(etype=etype, X=X, dM=dM, vals=vals, coeff=coeff, etype_t=etype[p["map_t"]], vals_t=None if vals is None else vals[p["map_t"]])
    d["M"] = spmm_typed_ref(p["rowptr"], p["colidx"], etype, X, R, coeff, vals)
    d["dX"] = spmm_typed_bwd_ref(p["rowptr_t"], p["colidx_t"], d["etype_t"], dM, R, F, coeff, d["vals_t"])
    if B is not None:
        d["dC"], d["D"] = typed_coeff_grad_ref(p["rowptr"], p["colidx"], etype, dM, X, R, B, vals)
    return d


def run(env, graph, d, R, F):
    """(M, dX, dC or None) of the three calls on the device."""
    ops, opt = env["ops"], lambda a: None if a is None else dev(env, a)
    X, dM, coeff = dev(env, d["X"]), dev(env, d["dM"]), opt(d["coeff"])
    M = ops.spmm_typed(graph["d_rowptr"], graph["d_colidx"], dev(env, d["etype"]), X, R, coeff=coeff, vals=opt(d["vals"]))
    dX = ops.spmm_typed_bwd(graph["d_rowptr_t"], graph["d_colidx_t"], dev(env, d["etype_t"]), dM, R, F, coeff=coeff, vals_t=opt(d["vals_t"]))
    dC = None if coeff is None else ops.typed_coeff_grad(graph["d_rowptr"], graph["d_colidx"], dev(env, d["etype"]), dM, X, R, coeff,
                                                        vals=opt(d["vals"]))
    return host(M), host(dX), dC


@pytest.mark.parametrize("F,R,B,with_vals", CASES)
def test_bits_of_forward_backward_and_coefficient_gradient(env, graph, F, R, B, with_vals):
    d = data(F, R, B, with_vals)
    M, dX, dC = run(env, graph, d, R, F)
    assert np.array_equal(bits(M), bits(d["M"])) and np.array_equal(bits(dX), bits(d["dX"]))
    if B is None:
        assert not M[:, (R - 1) * F:].any() and not np.signbit(M[:, (R - 1) * F:]).any()      # the relation that never occurs: +0
    else:
        assert np.array_equal(bits(host(dC)), bits(d["dC"]))


@pytest.mark.parametrize("R,B,with_vals", [(R, B, True) for R, B in MODES] + [(3, None, False), (5, 2, False)])
def test_exact_values_equal_the_float64_evaluation(env, graph, R, B, with_vals):
    F, p = 20, pattern()
    d = data(F, R, B, with_vals, "exact")
    rows, cols, t = np.repeat(np.arange(N), np.diff(p["rowptr"])), p["colidx"].astype(np.int64), d["etype"].astype(np.int64)
    nb = R if B is None else B
    w = (np.eye(R) if B is None else d["coeff"].astype(np.float64))[t] * (1.0 if d["vals"] is None else d["vals"].astype(np.float64)[:, None])
    X64, dM64 = d["X"].astype(np.float64), d["dM"].astype(np.float64).reshape(N, nb, F)
    want, size = [], []
    for f in (lambda a: a, np.abs):          # the values, then the sums of |term| that bound every partial sum
        M, dX = np.zeros((N, nb, F)), np.zeros((N, F))
        np.add.at(M, rows, f(w)[:, :, None] * f(X64)[cols][:, None, :])
        np.add.at(dX, cols, (f(w)[:, :, None] * f(dM64)[rows]).sum(1))
        dots = (f(dM64)[rows] * f(X64)[cols][:, None, :]).sum(2) * (1.0 if d["vals"] is None else d["vals"][:, None])
        dC = np.zeros((R, nb))
        np.add.at(dC, t, dots)
        (want if f is not np.abs else size).append((M.reshape(N, nb * F), dX, dC))
    assert max(a.max() for a in size[0]) < 2 ** 23           # multiples of 1/2 below 2^23: every float32 partial sum is exact
    M, dX, dC = run(env, graph, d, R, F)
    assert np.array_equal(M, want[0][0]) and np.array_equal(d["M"], want[0][0])
    assert np.array_equal(dX, want[0][1]) and np.array_equal(d["dX"], want[0][1])
    if B is not None:
        assert np.array_equal(host(dC), want[0][2]) and np.array_equal(d["dC"], want[0][2])


def test_one_hot_keeps_an_infinity_in_its_relation(env, graph):
    ops, p, F, R = env["ops"], pattern(), 16, 3
    col = int(p["colidx"][p["rowptr"][300]])                  # a column that some row names
    etype = np.where(p["colidx"] == col, 0, np.random.default_rng(5).integers(0, R, p["nnz"])).astype(np.int32)
    X = synth.uniform_pm1(9, (N, F))
    X[col] = np.inf
    M = host(ops.spmm_typed(graph["d_rowptr"], graph["d_colidx"], dev(env, etype), dev(env, X), R)).reshape(N, R, F)
    assert np.isinf(M[:, 0]).any() and np.isfinite(M[:, 1:]).all()


@pytest.mark.parametrize("layout", ("x_off", "odd_ldx", "m_off", "odd_ldm"))
def test_forward_bits_when_one_vec4_condition_fails(env, graph, layout):
    torch, F, R = env["torch"], 64, 3
    d = data(F, R, None, True)
    X = placed(env, d["X"], ld=F + 1 if layout == "odd_ldx" else None, off=1 if layout == "x_off" else 0)
    M, buf = strided(env, N, R * F, torch.float32, float("nan"), ld=R * F + 1 if layout == "odd_ldm" else None, off=1 if layout == "m_off" else 0)
    env["ops"].spmm_typed(graph["d_rowptr"], graph["d_colidx"], dev(env, d["etype"]), X, R, vals=dev(env, d["vals"]), out=M)
    assert np.array_equal(bits(host(M)), bits(d["M"]))        # beta = 0: no NaN of the prefilled M is read
    if layout == "odd_ldm":
        assert bool(torch.isnan(buf.view(N, R * F + 1)[:, R * F]).all())


def test_declines(env, graph):
    ops, capi, torch, p = env["ops"], env["capi"], env["torch"], pattern()
    etype, X = dev(env, np.zeros(p["nnz"], dtype=np.int32)), dev(env, np.zeros((N, 4), dtype=np.float32))
    with pytest.raises(capi.GnnxError, match="one slab per relation"):       # one-hot mode with 2 slabs for 3 relations
        ops.spmm_typed(graph["d_rowptr"], graph["d_colidx"], etype, X, 3, out=torch.empty((N, 8), device=env["dev"]))
    M, ws = torch.empty((N, 12), device=env["dev"]), torch.empty(64, dtype=torch.uint8, device=env["dev"])
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with pytest.raises(capi.GnnxError, match="n_slabs == n_types") as err:  # the same through the C-ABI: C == NULL with B != R
        capi.call("gnnx_spmm_csr_typed_f32", N, N, 4, p["nnz"], 3, 2, ptr(graph["d_rowptr"]), ptr(graph["d_colidx"]), ptr(etype), None, None,
                  ptr(X), 4, ptr(M), 12, ptr(ws), 64, None)
    assert err.value.status == -1
    with pytest.raises(capi.GnnxError) as err:
        capi.call("gnnx_spmm_csr_typed_f32", N, N, 4, p["nnz"], 3, 3, ptr(graph["d_rowptr"]), ptr(graph["d_colidx"]), ptr(etype), None, None,
                  ptr(X), 4, ptr(M), 12, ptr(ws), 64, None)
    assert err.value.status == -4
    g = ops.CsrGraph(N, graph["d_rowptr"], graph["d_colidx"])
    rows = dev(env, np.repeat(np.arange(N), np.diff(p["rowptr"])).astype(np.int32))
    with pytest.raises(capi.GnnxError, match=r"outside \[0, 4\)"):
        g.set_edge_type(rows, graph["d_colidx"], torch.full((p["nnz"],), 4, dtype=torch.int32, device=env["dev"]), 4)
