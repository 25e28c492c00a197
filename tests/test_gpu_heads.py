"""GPU tests of the multi-head calls (run with -m gpu on an MI355X): gnnx_spmm_csr_heads_f32, gnnx_sddmm_csr_heads_f32,
gnnx_csr_rowsum_heads_f32 and the heads edge softmax through ops.spmm_heads / sddmm_heads / csr_rowsum_heads / edge_softmax_heads /
edge_softmax_heads_bwd.

Every comparison is bit equality.  The aggregation and the scores are held to the NumPy restatements of tests/heads_ref.py (which
tests/test_heads_cpu.py shows equal to the single-head restatements head by head).  The softmax is held to the existing DEVICE
single-head call on contiguous copies of head h -- x goes through the device's own expf, so that call is the exact oracle -- and its
backward to the NumPy restatement as well.

Pattern A (tests/edge_softmax_ref.py): one row of every length 0 .. 12 293 that meets a boundary of an order or a kernel, hubs between
runs of short and empty rows, 16 384 columns.  Pattern B: tests/sddmm_ref.py random_csr with 2^10 rows and columns and 8000 draws.
Cells (H, D): a 256-wide single head; 8 x 8, 4 x 16, 2 x 64, 8 x 32 (16-byte pieces, 16 to 64 lanes per row); 8 x 64 (512 wide: two
feature tiles in the aggregation, two passes over an entry in the scores); 4 x 6 (a 4-float piece would straddle two heads); 3 x 5 (odd
everything); 8 x 1 (the per-head row sum); and 8 x 8 placed so that each vec4 condition fails in turn."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import heads_ref as hr
from tests import helpers  # noqa: F401  (registers the in-tree package as gnncpp_amd: the file also runs on its own)
from tests import sddmm_ref as sr

pytestmark = pytest.mark.gpu

CELLS = ((1, 256), (8, 8), (4, 16), (2, 64), (8, 32), (8, 64), (4, 6), (3, 5), (8, 1))
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
    rp_a, ci_a, _ = er.pattern_a()
    rp_b, ci_b = sr.random_csr(1, 1 << 10, 1 << 10, 8000)
    out = {}
    for name, rp, ci, n_cols in (("A", rp_a, ci_a, er.N_COLS_A), ("B", rp_b, ci_b, 1 << 10)):
        out[name] = dict(rowptr=rp, colidx=ci, n_rows=len(rp) - 1, n_cols=n_cols, nnz=len(ci), rowptr_d=dev(env, rp), colidx_d=dev(env, ci))
    assert (np.diff(rp_b) == 0).any() and int(np.diff(rp_b).max()) > 16   # empty rows, and rows beyond the short-row kernel's 16 lanes
    return out


def placed(env, a, ld=None, offset=0, fill=np.nan):
    """A device copy of the 2-D float32 array `a` as a view of leading dimension ld, `offset` floats into a 16-byte aligned buffer; the
    margins hold `fill`.  Returns (view, whole buffer)."""
    torch = env["torch"]
    n, f = a.shape
    ld = f if ld is None else ld
    buf = torch.full((n * ld + offset + 4,), fill, dtype=torch.float32, device=env["dev"])
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n * ld].view(n, ld)[:, :f]
    view.copy_(dev(env, a))
    return view, buf


def operands(P, H, D):
    rng = np.random.default_rng(100 * H + D + P["nnz"])
    u = lambda *shape: rng.uniform(-1, 1, shape).astype(np.float32)  # noqa: E731
    return dict(X=u(P["n_cols"], H * D), L=u(P["n_rows"], H * D), vals=u(P["nnz"], H), bias=u(H * D), y0=u(P["n_rows"], H * D))


def check_margins(buf, view_shape, ld, offset, before):
    """every float of the buffer outside the view kept its bits"""
    n, f = view_shape
    mask = np.ones(buf.numel(), dtype=bool)
    idx = offset + (np.arange(n)[:, None] * ld + np.arange(f)[None, :])
    mask[idx.ravel()] = False
    assert np.array_equal(host(buf).view(np.uint32)[mask], before.view(np.uint32)[mask])


@pytest.mark.parametrize("H,D", CELLS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_aggregation_bits(env, patterns, name, H, D):
    ops, P = env["ops"], patterns[name]
    op = operands(P, H, D)
    F = H * D
    X, vals = dev(env, op["X"]), dev(env, op["vals"])
    plain = ops.spmm_heads(P["rowptr_d"], P["colidx_d"], X, vals, H)
    assert np.array_equal(host(plain), hr.spmm_heads_ref(P["rowptr"], P["colidx"], op["X"], op["vals"], H))
    assert env["torch"].equal(plain, ops.spmm_heads(P["rowptr_d"], P["colidx_d"], X, vals, H))
    # everything at once: ldv > H, wide ldx / ldy (multiples of 4: the 16-byte path stays where D allows it), bias, beta = 1 onto a
    # prefilled Y whose margins must stay untouched, the ReLU
    Xw, _ = placed(env, op["X"], ld=F + 8)
    vw, _ = placed(env, op["vals"], ld=H + 3)
    Yw, Ybuf = placed(env, op["y0"], ld=F + 12, fill=7.0)
    before = host(Ybuf).copy()
    ops.spmm_heads(P["rowptr_d"], P["colidx_d"], Xw, vw, H, bias=dev(env, op["bias"]), beta=1.0, relu_out=True, out=Yw)
    want = hr.spmm_heads_ref(P["rowptr"], P["colidx"], op["X"], op["vals"], H, bias=op["bias"], y0=op["y0"], relu_out=True)
    assert np.array_equal(host(Yw), want)
    assert (want == 0).any() and (want > 0).any()
    check_margins(Ybuf, (P["n_rows"], F), F + 12, 0, before)


@pytest.mark.parametrize("fail", ["X pointer", "ldx", "Y pointer", "ldy", "bias pointer"])
def test_aggregation_scalar_lanes_when_a_vec4_condition_fails(env, patterns, fail):
    """8 x 8 placed so that one condition of the 16-byte path fails: the scalar lanes give the same bits, with and without the bias."""
    ops, P = env["ops"], patterns["B"]
    H, D, F = 8, 8, 64
    op = operands(P, H, D)
    Xv, _ = placed(env, op["X"], ld=F + (1 if fail == "ldx" else 0), offset=1 if fail == "X pointer" else 0)
    ldy, offy = F + (2 if fail == "ldy" else 0), (3 if fail == "Y pointer" else 0)
    Yv, Ybuf = placed(env, op["y0"], ld=ldy, offset=offy, fill=7.0)
    bias = placed(env, op["bias"][None, :], offset=1 if fail == "bias pointer" else 0)[0][0]
    assert any(t.data_ptr() % 16 for t in (Xv, Yv, bias)) or Xv.stride(0) % 4 or Yv.stride(0) % 4
    before = host(Ybuf).copy()
    ops.spmm_heads(P["rowptr_d"], P["colidx_d"], Xv, dev(env, op["vals"]), H, bias=bias, beta=1.0, out=Yv)
    assert np.array_equal(host(Yv), hr.spmm_heads_ref(P["rowptr"], P["colidx"], op["X"], op["vals"], H, bias=op["bias"], y0=op["y0"]))
    check_margins(Ybuf, (P["n_rows"], F), ldy, offy, before)
    if fail != "bias pointer":
        ops.spmm_heads(P["rowptr_d"], P["colidx_d"], Xv, dev(env, op["vals"]), H, out=Yv)
        assert np.array_equal(host(Yv), hr.spmm_heads_ref(P["rowptr"], P["colidx"], op["X"], op["vals"], H))


def test_head_dim_one_over_ones_is_the_descending_row_sum_and_rowsum_heads_the_ascending(env, patterns):
    ops, torch = env["ops"], env["torch"]
    for name in ("A", "B"):
        P = patterns[name]
        H = 8
        vals = operands(P, H, 1)["vals"]
        ones = torch.ones((P["n_cols"], H), dtype=torch.float32, device=env["dev"])
        wide, buf = placed(env, np.zeros((P["n_rows"], H), dtype=np.float32), ld=2 * H, offset=H, fill=3.0)   # the right half of [n, 2H]
        before = host(buf).copy()
        ops.spmm_heads(P["rowptr_d"], P["colidx_d"], ones, dev(env, vals), H, out=wide)
        rows = er.row_of_entries(P["rowptr"])
        down = np.zeros((P["n_rows"], H), dtype=np.float32)
        for p in range(P["nnz"] - 1, -1, -1):
            down[rows[p]] = down[rows[p]] + vals[p]
        assert np.array_equal(host(wide), down)
        check_margins(buf, (P["n_rows"], H), 2 * H, H, before)
        up = np.zeros((P["n_rows"], H), dtype=np.float32)
        for p in range(P["nnz"]):
            up[rows[p]] = up[rows[p]] + vals[p]
        vw, _ = placed(env, vals, ld=H + 1)
        ops.csr_rowsum_heads(P["rowptr_d"], vw, out=wide)
        assert np.array_equal(host(wide), up)
        check_margins(buf, (P["n_rows"], H), 2 * H, H, before)
        for h in range(H):   # column h carries the bits of the single-head call
            assert torch.equal(wide[:, h], ops.csr_rowsum(P["rowptr_d"], dev(env, vals[:, h])))
        assert not np.array_equal(up, down)   # the two orders are told apart


@pytest.mark.parametrize("H,D", CELLS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_scores_bits(env, patterns, name, H, D):
    """Rows of every length of pattern A (the non-zero domain: lane groups start and end inside rows and cross empty rows)."""
    ops, P = env["ops"], patterns[name]
    op = operands(P, H, D)
    L, R = dev(env, op["L"]), dev(env, op["X"])
    want = hr.sddmm_heads_ref(P["rowptr"], P["colidx"], op["L"], op["X"], H)
    got = ops.sddmm_heads(P["rowptr_d"], P["colidx_d"], L, R, H)
    assert np.array_equal(host(got), want)
    out, buf = placed(env, np.zeros((P["nnz"], H), dtype=np.float32), ld=H + 5, fill=9.0)   # ldo > H: the margins stay
    before = host(buf).copy()
    Lw, _ = placed(env, op["L"], ld=H * D + 4)
    ops.sddmm_heads(P["rowptr_d"], P["colidx_d"], Lw, R, H, out=out)
    assert np.array_equal(host(out), want)
    check_margins(buf, (P["nnz"], H), H + 5, 0, before)


@pytest.mark.parametrize("fail", ["L pointer", "ldl", "R pointer", "ldr"])
def test_scores_scalar_loads_when_a_vec4_condition_fails(env, patterns, fail):
    ops, P = env["ops"], patterns["B"]
    H, D, F = 8, 8, 64
    op = operands(P, H, D)
    Lv, _ = placed(env, op["L"], ld=F + (1 if fail == "ldl" else 0), offset=1 if fail == "L pointer" else 0)
    Rv, _ = placed(env, op["X"], ld=F + (3 if fail == "ldr" else 0), offset=2 if fail == "R pointer" else 0)
    assert Lv.data_ptr() % 16 or Rv.data_ptr() % 16 or Lv.stride(0) % 4 or Rv.stride(0) % 4
    got = ops.sddmm_heads(P["rowptr_d"], P["colidx_d"], Lv, Rv, H)
    assert np.array_equal(host(got), hr.sddmm_heads_ref(P["rowptr"], P["colidx"], op["L"], op["X"], H))


def test_scores_of_a_square_pattern_with_l_is_r_and_of_an_empty_pattern(env, patterns):
    ops, torch, P = env["ops"], env["torch"], patterns["B"]
    Z = operands(P, 4, 16)["X"]
    Zd = dev(env, Z)
    got = ops.sddmm_heads(P["rowptr_d"], P["colidx_d"], Zd, Zd, 4)
    assert np.array_equal(host(got), hr.sddmm_heads_ref(P["rowptr"], P["colidx"], Z, Z, 4))
    rp0 = torch.zeros(P["n_rows"] + 1, dtype=torch.int32, device=env["dev"])
    ci0 = torch.zeros(0, dtype=torch.int32, device=env["dev"])
    assert tuple(ops.sddmm_heads(rp0, ci0, Zd, Zd, 4).shape) == (0, 4)
    Y = ops.spmm_heads(rp0, ci0, Zd, torch.zeros((0, 4), dtype=torch.float32, device=env["dev"]), 4, bias=dev(env, Z[0]))
    assert np.array_equal(host(Y), np.broadcast_to(Z[0], Z.shape))   # every row empty: the bias alone


# ---- softmax ---------------------------------------------------------------------------------------------------------------------
def softmax_operands(env, P, H, mode, strided):
    """Host operands [*, H] and their device forms.  strided: scores / dalpha with a leading dimension above H, the terms the two
    halves of one [N, 2H] matrix when the pattern is square, else two arrays of row stride H + 2."""
    s, t, slope = MODES[mode]
    rng = np.random.default_rng(31 * H + P["nnz"])
    h = dict(scores=rng.uniform(-2, 2, (P["nnz"], H)).astype(np.float32) if s else None,
             rowterm=rng.uniform(-2, 2, (P["n_rows"], H)).astype(np.float32) if t else None,
             colterm=rng.uniform(-2, 2, (P["n_cols"], H)).astype(np.float32) if t else None)
    dalpha = rng.uniform(-1, 1, (P["nnz"], H)).astype(np.float32)
    if not strided:
        d = {k: None if v is None else dev(env, v) for k, v in h.items()}
        return h, d, dev(env, dalpha), dalpha, slope
    d = dict(scores=None if not s else placed(env, h["scores"], ld=H + 3)[0], rowterm=None, colterm=None)
    if t and P["n_rows"] == P["n_cols"]:
        ER = dev(env, np.concatenate([h["rowterm"], h["colterm"]], axis=1))
        d.update(rowterm=ER[:, :H], colterm=ER[:, H:])
    elif t:
        d.update(rowterm=placed(env, h["rowterm"], ld=H + 2)[0], colterm=placed(env, h["colterm"], ld=H + 2)[0])
    return h, d, placed(env, dalpha, ld=H + 1)[0], dalpha, slope


def column_d(env, d, hd):
    return {k: None if v is None else v[:, hd].contiguous() for k, v in d.items()}


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_softmax_forward_and_backward_bits(env, patterns, name, H, mode, strided):
    ops, torch, P = env["ops"], env["torch"], patterns[name]
    h, d, dalpha_d, dalpha, slope = softmax_operands(env, P, H, mode, strided)
    rp, ci = P["rowptr_d"], P["colidx_d"]
    x, m, z = ops.edge_softmax_heads(rp, ci, H, negative_slope=slope, unnormalised=True, want_stats=True, **d)
    if strided:   # alpha into a wider array; the margins stay
        alpha, abuf = placed(env, np.zeros((P["nnz"], H), dtype=np.float32), ld=H + 2, fill=5.0)
        before = host(abuf).copy()
        _, m2, z2 = ops.edge_softmax_heads(rp, ci, H, negative_slope=slope, want_stats=True, out=alpha, **d)
        check_margins(abuf, (P["nnz"], H), H + 2, 0, before)
    else:
        alpha, m2, z2 = ops.edge_softmax_heads(rp, ci, H, negative_slope=slope, want_stats=True, **d)
    assert torch.equal(m, m2) and torch.equal(z, z2)
    empty = np.diff(P["rowptr"]) == 0
    assert empty.any() and np.isneginf(host(m)[empty]).all() and (host(z)[empty] == 0).all() and not np.signbit(host(z)[empty]).any()
    drow_w, dbuf = placed(env, np.zeros((P["n_rows"], H), dtype=np.float32), ld=2 * H, fill=4.0)   # the left half of [n, 2H]
    before = host(dbuf).copy()
    dt, _ = ops.edge_softmax_heads_bwd(rp, ci, H, alpha, dalpha_d, negative_slope=slope, drowterm_out=drow_w, **d)
    check_margins(dbuf, (P["n_rows"], H), 2 * H, 0, before)
    for hd in range(H):   # the device's single-head call on contiguous copies of head hd
        kw = column_d(env, d, hd)
        x1, m1, z1 = ops.edge_softmax(rp, ci, negative_slope=slope, unnormalised=True, want_stats=True, **kw)
        a1 = ops.edge_softmax(rp, ci, negative_slope=slope, **kw)
        assert torch.equal(x[:, hd], x1) and torch.equal(m[:, hd], m1) and torch.equal(z[:, hd], z1), f"head {hd}: forward"
        assert torch.equal(alpha[:, hd], a1), f"head {hd}: alpha"
        dt1, drow1 = ops.edge_softmax_bwd(rp, ci, a1, dalpha_d[:, hd].contiguous(), negative_slope=slope, **kw)
        assert torch.equal(dt[:, hd], dt1) and torch.equal(drow_w[:, hd], drow1), f"head {hd}: backward"
    dt_ref, drow_ref = hr.edge_softmax_heads_bwd_ref(P["rowptr"], P["colidx"], host(alpha), dalpha, slope=slope, **h)
    assert np.array_equal(host(dt), dt_ref) and np.array_equal(host(drow_w), drow_ref)
    # the same bits every run
    dt2, drow2 = ops.edge_softmax_heads_bwd(rp, ci, H, alpha, dalpha_d, negative_slope=slope, **d)
    assert torch.equal(dt2, dt) and torch.equal(drow2, drow_w)
    assert torch.equal(ops.edge_softmax_heads(rp, ci, H, negative_slope=slope, unnormalised=True, **d), x)


def test_softmax_workspace(env, patterns):
    capi, torch, P = env["capi"], env["torch"], patterns["A"]
    sizes = {}
    for H in (1, 3, 8):
        b = C.c_size_t(0)
        capi.call("gnnx_edge_softmax_heads_workspace", P["n_rows"], P["nnz"], H, C.byref(b))
        sizes[H] = b.value
    single = C.c_size_t(0)
    capi.call("gnnx_edge_softmax_workspace", P["n_rows"], P["nnz"], C.byref(single))
    assert sizes[1] == single.value and sizes[1] < sizes[3] < sizes[8] and sizes[8] % 256 == 0
    H = 8
    rt = torch.zeros((P["n_rows"], H), dtype=torch.float32, device=env["dev"])
    out = torch.empty((P["nnz"], H), dtype=torch.float32, device=env["dev"])
    ws = torch.empty(sizes[8], dtype=torch.uint8, device=env["dev"])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda nbytes: (P["n_rows"], P["n_cols"], P["nnz"], p(P["rowptr_d"]), p(P["colidx_d"]), H, None, H, p(rt), H, None, 0, 0.2, 0,  # noqa: E731
                           p(out), H, None, None, p(ws), nbytes, None)
    with pytest.raises(capi.GnnxError) as e:
        capi.call("gnnx_edge_softmax_csr_heads_f32", *args(sizes[8] - 256))
    assert e.value.status == -4
    capi.call("gnnx_edge_softmax_csr_heads_f32", *args(sizes[8]))
    torch.cuda.synchronize()
    deg = np.diff(P["rowptr"])
    want = np.repeat(np.float32(1) / deg[deg > 0].astype(np.float32), deg[deg > 0])   # equal scores: alpha = 1 / d, one division
    assert np.array_equal(host(out), want[:, None].repeat(H, 1))
