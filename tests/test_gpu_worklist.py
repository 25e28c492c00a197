"""GPU test of the hub list that the edge softmax, the neighbourhood reductions and the sampler share (gnnx_worklist.h; run with -m gpu
on an MI355X): ONE pattern with four hubs of different segment counts goes through all three units, so that a slip in the shared
listing or slot arithmetic (a hub's first slot, the slot -> (hub, segment) step, the last segment's length) shows in every consumer.

The pattern: 13 000 columns; hubs of S + 1, 2 S, 2 S + 1 and 3 S + 7 entries (2, 2, 3 and 4 segments: 11 slots, last segments of 1, S,
1 and 7 entries) between an empty row, rows of 1 .. 16 entries (the short-row kernels), of 17 .. 300 (the long-row lists of the
softmax and, past 256, of the sampler) and one of exactly S.  The reductions' backward walks the TRANSPOSED pattern, whose rows are
this pattern's columns; to give it the same hubs the pattern itself is taken as the transposed one, i.e. the backward is that of
A = P^T.  Every comparison is the one the unit's own suite makes (tests/test_gpu_edge_softmax.py, test_gpu_heads.py,
test_gpu_reduce.py, test_gpu_sample.py) against the same references; every call runs twice and the two results are torch.equal: the
order in which hubs land in the list may differ between calls, the values may not."""
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import heads_ref as hr
from tests.helpers import assert_close, synth
from tests.reduce_ref import SEG, spmm_reduce_bwd_ref, spmm_reduce_ref, transpose_csr
from tests.sample_ref import sample_ref

pytestmark = pytest.mark.gpu

S = SEG
N_COLS = 13000
HUBS = {1: S + 1, 4: 2 * S, 7: 2 * S + 1, 10: 3 * S + 7}
LENGTHS = [3, S + 1, 0, 300, 2 * S, 17, 16, 2 * S + 1, 1, 257, 3 * S + 7, 5, 64, S, 40, 256, 2, 0, 9]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    return dict(torch=torch, ops=ops, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def P(env):
    """The pattern on the host and on the device, and A = P^T with the map that makes P the transposed pattern of A; never changed."""
    assert S == 4096 and all(LENGTHS[r] == d for r, d in HUBS.items()) and max(LENGTHS) <= N_COLS
    rng = np.random.default_rng(77)
    rowptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.permutation(N_COLS)[:d]) for d in LENGTHS]).astype(np.int32)
    rowptr_a, colidx_a, _ = transpose_csr(rowptr, colidx, N_COLS)              # A = P^T: N_COLS rows, len(LENGTHS) columns
    rowptr_t, colidx_t, map_t = transpose_csr(rowptr_a, colidx_a, len(LENGTHS))   # its transposed pattern is P again
    assert np.array_equal(rowptr_t, rowptr) and np.array_equal(colidx_t, colidx)
    deg = np.diff(rowptr)
    assert sorted(-(-d // S) for d in deg[deg > S]) == [2, 2, 3, 4] and (deg == 0).any() and (deg == S).any()
    out = dict(rowptr=rowptr, colidx=colidx, nnz=len(colidx), n_rows=len(LENGTHS), rowptr_a=rowptr_a, colidx_a=colidx_a, map_t=map_t)
    for k in ("rowptr", "colidx", "rowptr_a", "colidx_a", "map_t"):
        out["d_" + k] = dev(env, out[k])
    return out


def ulps(x, x64):
    """the error of float32 x against float64 x64 in float32 ulps of x64, where x64 is a normal float32"""
    normal = x64 >= 2.0 ** -126
    err = np.abs(x.astype(np.float64) - x64)[normal] / np.spacing(x64[normal].astype(np.float32)).astype(np.float64)
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("H", [1, 3])
def test_edge_softmax_forward_and_backward(env, P, H):
    ops, torch = env["ops"], env["torch"]
    rp, ci, slope = P["rowptr"], P["colidx"], 0.2
    rng = np.random.default_rng(10 + H)
    h = dict(scores=rng.uniform(-2, 2, (P["nnz"], H)).astype(np.float32), rowterm=rng.uniform(-2, 2, (P["n_rows"], H)).astype(np.float32),
             colterm=rng.uniform(-2, 2, (N_COLS, H)).astype(np.float32))
    dalpha = rng.uniform(-1, 1, (P["nnz"], H)).astype(np.float32)
    d = {k: dev(env, v) for k, v in h.items()}
    d_dalpha = dev(env, dalpha)

    def forward(unnormalised):
        return ops.edge_softmax_heads(P["d_rowptr"], P["d_colidx"], H, negative_slope=slope, unnormalised=unnormalised, want_stats=True, **d)

    x_d, m_d, z_d = forward(True)
    x, m, z = host(x_d), host(m_d), host(z_d)
    arg, m_ref = hr.exp_argument_heads(er.leaky(hr.pre_activation_heads(rp, ci, **h), slope), rp)
    empty = np.diff(rp) == 0
    assert np.array_equal(m, m_ref), "rowmax"
    assert np.isneginf(m[empty]).all() and (z[empty] == 0).all() and not np.signbit(z[empty]).any()
    x64 = np.exp(arg.astype(np.float64))
    worst = ulps(x, x64)
    print(f"H = {H}: expf within {worst:.3f} ulp of float64 exp of the same argument")
    assert_close(x, x64, "x")
    assert worst <= 2.0, f"expf off by {worst:.3f} ulp"
    assert np.array_equal(z, hr.row_sum_in_order_heads(x, rp)), "rowsum is not the restated sum of the device's own x"
    a_d, m2, z2 = forward(False)
    assert np.array_equal(host(a_d), hr.edge_softmax_heads_from_x(x, z, rp)), "alpha is not x / z"
    assert torch.equal(m2, m_d) and torch.equal(z2, z_d)
    for first, again in zip((x_d, m_d, z_d, a_d), forward(True) + (forward(False)[0],)):
        assert torch.equal(first, again), "forward: a second call gives other bits"

    def backward():
        return ops.edge_softmax_heads_bwd(P["d_rowptr"], P["d_colidx"], H, a_d, d_dalpha, negative_slope=slope, **d)

    dt_d, drow_d = backward()
    dt_ref, drow_ref = hr.edge_softmax_heads_bwd_ref(rp, ci, host(a_d), dalpha, slope=slope, **h)
    assert np.array_equal(host(dt_d), dt_ref), "dt"
    assert np.array_equal(host(drow_d), drow_ref), "drowterm"
    dt2, drow2 = backward()
    assert torch.equal(dt2, dt_d) and torch.equal(drow2, drow_d), "backward: a second call gives other bits"
    if H == 1:   # the single-head entry points are the same code at H = 1
        kw = {k: v[:, 0].contiguous() for k, v in d.items()}
        assert torch.equal(ops.edge_softmax(P["d_rowptr"], P["d_colidx"], negative_slope=slope, **kw), a_d[:, 0])
        dt1, drow1 = ops.edge_softmax_bwd(P["d_rowptr"], P["d_colidx"], a_d[:, 0].contiguous(), d_dalpha[:, 0].contiguous(), negative_slope=slope, **kw)
        assert torch.equal(dt1, dt_d[:, 0]) and torch.equal(drow1, drow_d[:, 0])


@pytest.mark.parametrize("F", [4, 5])
def test_spmm_reduce_forward_and_backward(env, P, F):
    """F = 4: the float4 pieces; F = 5: the scalar ones.  Values with ties and signed zeros, as in tests/test_gpu_reduce.py."""
    ops, torch = env["ops"], env["torch"]
    rng = np.random.default_rng(20 + F)
    X = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32), size=(N_COLS, F))
    vals = rng.choice(np.array([-1, 0.5, 1], dtype=np.float32), size=P["nnz"])
    d_X, d_vals = dev(env, X), dev(env, vals)
    for op in ("max", "min"):
        for v, d_v in ((None, None), (vals, d_vals)):
            Y, arg = ops.spmm_reduce(P["d_rowptr"], P["d_colidx"], d_X, op=op, vals=d_v)
            Yr, argr = spmm_reduce_ref(P["rowptr"], P["colidx"], X, v, op)
            what = f"forward {op} vals={v is not None}"
            assert np.array_equal(host(arg), argr), what
            assert np.array_equal(bits(host(Y)), bits(Yr)), what
            Y2, arg2 = ops.spmm_reduce(P["d_rowptr"], P["d_colidx"], d_X, op=op, vals=d_v)
            assert torch.equal(Y2, Y) and torch.equal(arg2, arg), what + ": a second call gives other bits"
    # backward of A = P^T: P is its transposed pattern, vals and arg are in the order of CSR(A)
    XA = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32), size=(P["n_rows"], F))
    G, y0 = synth.uniform_pm1(33 + F, (N_COLS, F)), synth.uniform_pm1(34 + F, (P["n_rows"], F))
    d_G = dev(env, G)
    for v, d_v in ((None, None), (vals, d_vals)):
        _, arg = spmm_reduce_ref(P["rowptr_a"], P["colidx_a"], XA, v, "max")
        d_arg = dev(env, arg)
        for beta in (0, 1):
            def backward():
                dX = dev(env, y0) if beta else torch.full((P["n_rows"], F), float("nan"), dtype=torch.float32, device=env["dev"])
                ops.spmm_reduce_bwd(P["d_rowptr"], P["d_colidx"], P["d_map_t"], d_arg, d_G, vals=d_v, out=dX, beta=float(beta))
                return dX
            dX = backward()
            ref = spmm_reduce_bwd_ref(P["rowptr"], P["colidx"], P["map_t"], arg, G, v, y0 if beta else None)
            what = f"backward vals={v is not None} beta={beta}"
            assert np.isfinite(host(dX)).all(), what
            assert np.array_equal(bits(host(dX)), bits(ref)), what
            assert torch.equal(backward(), dX), what + ": a second call gives other bits"


def test_sample_neighbors(env, P):
    ops, torch = env["ops"], env["torch"]
    k, seed = 5, 0xDEADBEEF12345678
    got = ops.sample_neighbors(P["d_rowptr"], P["d_colidx"], k, seed, want_pos=True, want_rowid=True)
    ref = sample_ref(P["rowptr"], P["colidx"], k, seed)
    for name, g, r in zip(("rowptr", "colidx", "pos", "rowid"), got, ref):
        assert host(g).dtype == np.int32 and np.array_equal(host(g), r), f"{name} differs from the reference"
    again = ops.sample_neighbors(P["d_rowptr"], P["d_colidx"], k, seed, want_pos=True, want_rowid=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "a second call gives other bits"
