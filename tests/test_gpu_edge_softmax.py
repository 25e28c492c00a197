"""GPU tests of the edge softmax (run with -m gpu on an MI355X): gnnx_edge_softmax_csr_f32 / gnnx_edge_softmax_bwd_csr_f32 through
ops.edge_softmax / ops.edge_softmax_bwd against the NumPy restatement tests/edge_softmax_ref.py.

Every comparison is bit equality (np.array_equal / torch.equal) except three, at the project bar tests.helpers.assert_close: the device's
own x = expf(e - m) against float64 exp of the SAME float32 argument (plus, wherever the float64 value is a normal float32, an error
of at most 2 ulp -- twice the 1 ulp the HIP math accuracy table gives expf); a row's alpha summing to 1; and the backward against
float64.  The row order is pinned independently of expf: rowsum must equal the restated sum of the device's own x.

Pattern A (tests/edge_softmax_ref.py pattern_a): 16 384 columns, one row of every length 0 .. 12 293 that meets a boundary of the
row order or of the kernels (16 | 17 lanes per row / a wavefront per row, 64 | 65 registers / three passes, 4096 | 4097 one row /
segments), hubs between runs of short and empty rows.  Pattern B: the R-MAT graph of tests/test_gpu_link.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import sddmm_ref as sr
from tests.helpers import assert_close, synth

pytestmark = pytest.mark.gpu

MODES = {"scores": (True, False, 1.0), "terms": (False, True, 0.2), "all": (True, True, 0.2)}   # (scores, terms, slope)


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


@pytest.fixture(scope="module")
def patterns(env):
    """name -> dict(rowptr, colidx, n_cols, operands on the host and on the device, transposed pattern); built once, never changed."""
    ops = env["ops"]
    rp_a, ci_a, _ = er.pattern_a()
    src, dst = synth.rmat_edges(91, 1 << 10, 8000)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), 1 << 10, norm=False)
    out = {}
    for name, rp, ci, n_cols in (("A", rp_a, ci_a, er.N_COLS_A), ("B", host(g.rowptr), host(g.colidx), 1 << 10)):
        rng = np.random.default_rng(len(ci))
        n_rows, nnz = len(rp) - 1, len(ci)
        rp_t, ci_t = sr.transpose_csr(rp, ci, n_cols)
        h = dict(scores=rng.uniform(-2, 2, nnz).astype(np.float32), rowterm=rng.uniform(-2, 2, n_rows).astype(np.float32),
                 colterm=rng.uniform(-2, 2, n_cols).astype(np.float32), dalpha=rng.uniform(-1, 1, nnz).astype(np.float32))
        out[name] = dict(rowptr=rp, colidx=ci, n_cols=n_cols, n_rows=n_rows, nnz=nnz, h=h, d={k: dev(env, v) for k, v in h.items()},
                         rowptr_d=dev(env, rp), colidx_d=dev(env, ci), rowptr_t=rp_t, colidx_t=ci_t)
    assert out["A"]["nnz"] > 40000 and int(np.diff(out["B"]["rowptr"]).max()) > 64 and (np.diff(out["B"]["rowptr"]) == 0).any()
    return out


def operands_of(P, mode, where):
    s, t, slope = MODES[mode]
    src = P[where]
    return dict(scores=src["scores"] if s else None, rowterm=src["rowterm"] if t else None, colterm=src["colterm"] if t else None), slope


def ulps(x, x64):
    """the error of float32 x against float64 x64 in float32 ulps of x64, where x64 is a normal float32"""
    normal = x64 >= 2.0 ** -126
    err = np.abs(x.astype(np.float64) - x64)[normal] / np.spacing(x64[normal].astype(np.float32)).astype(np.float64)
    return float(err.max()) if err.size else 0.0


def check_forward(env, P, kw_h, kw_d, slope, what):
    ops = env["ops"]
    rp, ci = P["rowptr"], P["colidx"]
    x_d, m_d, z_d = ops.edge_softmax(P["rowptr_d"], P["colidx_d"], negative_slope=slope, unnormalised=True, want_stats=True, **kw_d)
    x, m, z = host(x_d), host(m_d), host(z_d)
    e = er.leaky(er.pre_activation(rp, ci, **kw_h), slope)
    arg, m_ref = er.exp_argument(e, rp)
    assert np.array_equal(m, m_ref), f"{what}: rowmax"
    assert np.all(np.isneginf(m[np.diff(rp) == 0])) and np.all(z[np.diff(rp) == 0] == 0) and not np.signbit(z[np.diff(rp) == 0]).any()
    x64 = np.exp(arg.astype(np.float64))
    worst = ulps(x, x64)
    print(f"{what}: expf within {worst:.3f} ulp of float64 exp of the same argument")
    assert_close(x, x64, f"{what}: x")
    assert worst <= 2.0, f"{what}: expf off by {worst:.3f} ulp"
    assert np.array_equal(z, er.row_sum_in_order(x, rp)), f"{what}: rowsum is not the restated sum of the device's own x"
    a_d, m2, z2 = ops.edge_softmax(P["rowptr_d"], P["colidx_d"], negative_slope=slope, want_stats=True, **kw_d)
    assert np.array_equal(host(a_d), er.edge_softmax_from_x(x, z, rp)), f"{what}: alpha is not x / z"
    assert env["torch"].equal(m2, m_d) and env["torch"].equal(z2, z_d)
    assert env["torch"].equal(a_d, ops.edge_softmax(P["rowptr_d"], P["colidx_d"], negative_slope=slope, **kw_d))
    return a_d


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_bits(env, patterns, name, mode):
    P = patterns[name]
    kw_h, slope = operands_of(P, mode, "h")
    kw_d, _ = operands_of(P, mode, "d")
    check_forward(env, P, kw_h, kw_d, slope, f"pattern {name}, {mode}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_strided_terms_have_the_bits_of_contiguous_ones(env, patterns, name):
    """el and er as columns of [n, 2] matrices (stride 2) against contiguous copies, forward and backward."""
    torch, ops, P = env["torch"], env["ops"], patterns[name]
    R = torch.stack([P["d"]["rowterm"], torch.full_like(P["d"]["rowterm"], 7.0)], dim=1).contiguous()
    Cm = torch.stack([torch.full_like(P["d"]["colterm"], -7.0), P["d"]["colterm"]], dim=1).contiguous()
    assert R[:, 0].stride(0) == 2 and Cm[:, 1].stride(0) == 2 and Cm[:, 1].data_ptr() != Cm.data_ptr()
    rp, ci = P["rowptr_d"], P["colidx_d"]
    a_s = ops.edge_softmax(rp, ci, rowterm=R[:, 0], colterm=Cm[:, 1], negative_slope=0.2)
    a_c = ops.edge_softmax(rp, ci, rowterm=P["d"]["rowterm"], colterm=P["d"]["colterm"], negative_slope=0.2)
    assert torch.equal(a_s, a_c)
    got_s = ops.edge_softmax_bwd(rp, ci, a_c, P["d"]["dalpha"], rowterm=R[:, 0], colterm=Cm[:, 1], negative_slope=0.2)
    got_c = ops.edge_softmax_bwd(rp, ci, a_c, P["d"]["dalpha"], rowterm=P["d"]["rowterm"], colterm=P["d"]["colterm"], negative_slope=0.2)
    assert torch.equal(got_s[0], got_c[0]) and torch.equal(got_s[1], got_c[1])


def test_spread_logits_underflow_to_zero_and_stay_finite(env, patterns):
    """One row's logits run over +-60: x underflows to exactly 0 for some entries, every output is finite, alpha sums to 1."""
    ops, P = env["ops"], patterns["A"]
    rp = P["rowptr"]
    row = int(np.nonzero(np.diff(rp) == 257)[0][0])
    s = P["h"]["scores"].copy()
    s[rp[row]:rp[row + 1]] = np.linspace(-60, 60, 257).astype(np.float32)
    x, m, z = (host(t) for t in ops.edge_softmax(P["rowptr_d"], P["colidx_d"], scores=dev(env, s), unnormalised=True, want_stats=True))
    alpha = host(ops.edge_softmax(P["rowptr_d"], P["colidx_d"], scores=dev(env, s)))
    seg = slice(rp[row], rp[row + 1])
    assert m[row] == 60 and (x[seg] == 0).any() and x[seg].max() == 1
    assert np.isfinite(x).all() and np.isfinite(alpha).all() and np.isfinite(z).all()
    assert np.array_equal(alpha, er.edge_softmax_from_x(x, z, rp))
    assert_close(np.array([alpha[seg].astype(np.float64).sum()]), np.array([1.0]), "the spread row's alpha sums to 1")
    sums = np.add.reduceat(alpha.astype(np.float64), rp[:-1][np.diff(rp) > 0])
    assert_close(sums, np.ones_like(sums), "every row's alpha sums to 1")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_bits_and_float64(env, patterns, name, mode):
    """dt and drowterm equal the restatement bit for bit (slope 1 / 0.2, operands of both signs: both branches of the mask); dt, drowterm
    and the column-term gradient through csr_rowsum(rowptr_t, dt[map_t]) against float64."""
    ops, P = env["ops"], patterns[name]
    kw_h, slope = operands_of(P, mode, "h")
    kw_d, _ = operands_of(P, mode, "d")
    rp, ci = P["rowptr"], P["colidx"]
    t = er.pre_activation(rp, ci, **kw_h)
    assert (t > 0).any() and (t < 0).any()
    alpha_d = ops.edge_softmax(P["rowptr_d"], P["colidx_d"], negative_slope=slope, **kw_d)
    dt_d, drow_d = ops.edge_softmax_bwd(P["rowptr_d"], P["colidx_d"], alpha_d, P["d"]["dalpha"], negative_slope=slope, **kw_d)
    dt, drow = host(dt_d), host(drow_d)
    dt_ref, drow_ref = er.edge_softmax_bwd_ref(rp, ci, host(alpha_d), P["h"]["dalpha"], slope=slope, **kw_h)
    assert np.array_equal(dt, dt_ref), f"dt: {(dt != dt_ref).sum()} of {dt.size} entries differ"
    assert np.array_equal(drow, drow_ref), f"drowterm: rows {np.nonzero(drow != drow_ref)[0][:8]} differ"
    assert not np.signbit(drow[np.diff(rp) == 0]).any() and np.all(drow[np.diff(rp) == 0] == 0)
    # against float64: the whole chain, the column-term gradient included
    rp_t, ci_t = dev(env, P["rowptr_t"]), dev(env, P["colidx_t"])
    map_t = ops.csr_transpose_map(P["rowptr_d"], P["colidx_d"], rp_t, ci_t)
    assert np.array_equal(host(map_t), sr.transpose_map_ref(rp, ci, P["rowptr_t"], P["colidx_t"]))
    dcol = host(ops.csr_rowsum(rp_t, dt_d[map_t.long()].contiguous()))
    model = er.edge_softmax_ref64(rp, ci, P["n_cols"], slope=slope, dalpha=P["h"]["dalpha"], **kw_h)
    ent = er.row_of_entries(rp)
    assert_close(host(alpha_d), model["alpha"], "alpha")
    assert_close(dt, model["dt"], "dt", absum=model["absum"][ent])
    assert_close(drow, model["drowterm"], "drowterm", absum=2 * model["absum"])
    # |dt_p| <= 2 absum of its row, and dt_p itself is held to absum of its row above: a column's sum of them at the sum of those scales
    assert_close(dcol, model["dcolterm"], "dcolterm", absum=2 * np.bincount(ci.astype(np.int64), weights=model["absum"][ent], minlength=P["n_cols"]))


def raw_forward(env, P, ws_bytes, pad=0):
    """gnnx_edge_softmax_csr_f32 with a workspace of the caller's size (the bytes the call is TOLD; the buffer has `pad` more)."""
    torch, ops, capi = env["torch"], env["ops"], env["capi"]
    ws = torch.empty(max(ws_bytes + pad, 256), dtype=torch.uint8, device=env["dev"])
    out = torch.empty(P["nnz"], dtype=torch.float32, device=env["dev"])
    z = torch.empty(P["n_rows"], dtype=torch.float32, device=env["dev"])
    p = ops._ptr
    capi.call("gnnx_edge_softmax_csr_f32", P["n_rows"], P["n_cols"], P["nnz"], p(P["rowptr_d"]), p(P["colidx_d"]), p(P["d"]["scores"]),
              p(P["d"]["rowterm"]), 1, p(P["d"]["colterm"]), 1, 0.2, 0, p(out), None, p(z), p(ws), ws_bytes, ops._stream())
    return out, z


@pytest.mark.parametrize("name", ["A", "B"])
def test_repeatable_and_independent_of_the_workspace(env, patterns, name):
    torch, ops, capi, P = env["torch"], env["ops"], env["capi"], patterns[name]
    need = C.c_size_t(0)
    capi.call("gnnx_edge_softmax_workspace", P["n_rows"], P["nnz"], C.byref(need))
    a1, z1 = raw_forward(env, P, need.value)
    a2, z2 = raw_forward(env, P, need.value)
    a3, z3 = raw_forward(env, P, need.value + 4096)
    assert torch.equal(a1, a2) and torch.equal(z1, z2) and torch.equal(a1, a3) and torch.equal(z1, z3)
    assert torch.equal(a1, ops.edge_softmax(P["rowptr_d"], P["colidx_d"], negative_slope=0.2, **operands_of(P, "all", "d")[0]))
    with pytest.raises(capi.GnnxError) as ei:
        raw_forward(env, P, need.value - 1, pad=1)
    assert ei.value.status == -4
    b1 = ops.edge_softmax_bwd(P["rowptr_d"], P["colidx_d"], a1, P["d"]["dalpha"], negative_slope=0.2, **operands_of(P, "all", "d")[0])
    b2 = ops.edge_softmax_bwd(P["rowptr_d"], P["colidx_d"], a1, P["d"]["dalpha"], negative_slope=0.2, **operands_of(P, "all", "d")[0])
    assert torch.equal(b1[0], b2[0]) and torch.equal(b1[1], b2[1])


def test_no_entries_still_writes_the_row_outputs(env):
    torch, ops = env["torch"], env["ops"]
    rp = torch.zeros(6, dtype=torch.int32, device=env["dev"])
    ci = torch.empty(0, dtype=torch.int32, device=env["dev"])
    term = torch.ones(5, dtype=torch.float32, device=env["dev"])
    a, m, z = ops.edge_softmax(rp, ci, rowterm=term, want_stats=True)
    assert a.numel() == 0 and np.all(np.isneginf(host(m))) and np.all(host(z) == 0) and not np.signbit(host(z)).any()
    dt, drow = ops.edge_softmax_bwd(rp, ci, a, a, rowterm=term)
    assert dt.numel() == 0 and np.all(host(drow) == 0) and not np.signbit(host(drow)).any()
