"""GPU tests of the dynamic-attention calls (run with -m gpu on an MI355X): gnnx_gatv2_scores_csr_f32 and gnnx_gatv2_scores_bwd_csr_f32
through ops.gatv2_scores / ops.gatv2_scores_bwd, held to the NumPy restatement of tests/gatv2_ref.py with bit equality.

The pattern (gatv2_ref.make_pattern, 192 x 320): empty rows, rows of 1 .. 11 entries (several inside one group of 32 entries, rows that
end inside one), a row of 65 and one of 300 entries (each longer than a 64-wide window), nnz odd.  Cells: head_dim 1, 3, 4, 6, 8, 16, 64,
256, 260 (lane groups 1 .. 64; at 260 two chunks per lane) by n_heads 1, 2, 3, 8 where H D <= 2080.  Each cell runs contiguous, with
padded leading dimensions (NaN in the pads, sentinels around the outputs) and with every vec4 condition broken (a pointer one float off,
an odd leading dimension): the bits must not move.  The references of a cell are computed once and shared."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from tests import gatv2_ref as gr
from tests import helpers  # noqa: F401  (registers the in-tree package as gnncpp_amd: the file also runs on its own)
from tests import sddmm_ref as sr

pytestmark = pytest.mark.gpu

N_ROWS, N_COLS, SLOPE = 192, 320, 0.2
CELLS = [(H, D) for D in (1, 3, 4, 6, 8, 16, 64, 256, 260) for H in (1, 2, 3, 8) if H * D <= 2080]
INVALID_ARG = -1


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


@functools.lru_cache(maxsize=None)
def pattern(n_rows=N_ROWS, n_cols=N_COLS):
    rp, ci = gr.make_pattern(11, n_rows, n_cols)
    rp_t, ci_t = sr.transpose_csr(rp, ci, n_cols)
    deg = np.diff(rp)
    assert (deg == 0).any() and 65 in deg and 300 in deg and len(ci) % 32 and len(ci) % 4
    assert (rp[1:][deg > 0] % 32 != 0).any() and (np.diff(rp // 32) == 0).any()   # rows end inside a group; several rows in one group
    return dict(rowptr=rp, colidx=ci, rowptr_t=rp_t, colidx_t=ci_t, map_t=sr.transpose_map_ref(rp, ci, rp_t, ci_t), n_rows=n_rows,
                n_cols=n_cols, nnz=len(ci))


@pytest.fixture(scope="module")
def P(env):
    p = dict(pattern())
    for k in ("rowptr", "colidx", "rowptr_t", "colidx_t", "map_t"):
        p[k + "_d"] = dev(env, p[k])
    return p


@functools.lru_cache(maxsize=None)
def case(H, D):
    """Host operands of a cell and the restated results, computed once: out; (dL, T) on the forward pattern from +0; dR on the transposed
    pattern ADDED onto y0R, from de gathered into the transposed order by hand."""
    p = pattern()
    rng = np.random.default_rng(1000 * H + D)
    u = lambda *shape: rng.uniform(-1, 1, shape).astype(np.float32)  # noqa: E731
    F = H * D
    c = dict(L=u(p["n_rows"], F), R=u(p["n_cols"], F), a=u(F), de=u(p["nnz"], H), y0L=u(p["n_rows"], F), y0R=u(p["n_cols"], F))
    c["out"] = gr.scores_ref(p["rowptr"], p["colidx"], c["L"], c["R"], c["a"], H, SLOPE)
    c["dL"], c["T"] = gr.scores_bwd_ref(p["rowptr"], p["colidx"], c["de"], c["L"], c["R"], c["a"], H, SLOPE, want_T=True)
    c["dR1"], _ = gr.scores_bwd_ref(p["rowptr_t"], p["colidx_t"], c["de"][p["map_t"]], c["R"], c["L"], c["a"], H, SLOPE, y0=c["y0R"])
    u_all = c["L"][sr.row_of_entries(p["rowptr"])] + c["R"][p["colidx"]]
    assert (u_all > 0).any() and (u_all < 0).any()   # both branches
    return c


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


def check_margins(buf, view_shape, ld, offset, before):
    """every float of the buffer outside the view kept its bits"""
    n, f = view_shape
    mask = np.ones(buf.numel(), dtype=bool)
    idx = offset + (np.arange(n)[:, None] * ld + np.arange(f)[None, :])
    mask[idx.ravel()] = False
    assert np.array_equal(host(buf).view(np.uint32)[mask], before.view(np.uint32)[mask])


def odd(F):
    """an odd leading dimension >= F + 1"""
    return F + 1 + F % 2


@pytest.mark.parametrize("H,D", CELLS)
def test_scores_bits(env, P, H, D):
    ops, c, F = env["ops"], case(H, D), H * D
    L, R, a = dev(env, c["L"]), dev(env, c["R"]), dev(env, c["a"])
    got = ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], L, R, a, H, negative_slope=SLOPE)
    assert np.array_equal(host(got), c["out"])
    # padded leading dimensions (multiples of 4: the 16-byte path stays where D allows it), NaN in the pads, a sentinel around out
    Lw, _ = placed(env, c["L"], ld=F + 4)
    Rw, _ = placed(env, c["R"], ld=F + 8)
    out, buf = placed(env, np.zeros((P["nnz"], H), dtype=np.float32), ld=H + 3, fill=9.0)
    before = host(buf).copy()
    ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], Lw, Rw, a, H, negative_slope=SLOPE, out=out)
    assert np.array_equal(host(out), c["out"])
    check_margins(buf, (P["nnz"], H), H + 3, 0, before)
    # the scalar path for the same data: each vec4 condition broken in turn
    av = placed(env, c["a"][None, :], offset=1)[0][0]
    for Lv, Rv, avec in ((placed(env, c["L"], offset=1)[0], R, a), (L, placed(env, c["R"], offset=3)[0], a),
                         (placed(env, c["L"], ld=odd(F))[0], R, a), (L, placed(env, c["R"], ld=odd(F))[0], a), (L, R, av)):
        assert any(t.data_ptr() % 16 for t in (Lv, Rv, avec)) or Lv.stride(0) % 4 or Rv.stride(0) % 4
        assert env["torch"].equal(ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], Lv, Rv, avec, H, negative_slope=SLOPE), got)


@pytest.mark.parametrize("H,D", CELLS)
def test_backward_bits_on_the_forward_pattern(env, P, H, D):
    """entry_map = NULL: dL and T; T = NULL; beta = 0 and 1; padded and misaligned operands."""
    ops, torch, c, F = env["ops"], env["torch"], case(H, D), H * D
    rp, ci = P["rowptr_d"], P["colidx_d"]
    L, R, a, de = dev(env, c["L"]), dev(env, c["R"]), dev(env, c["a"]), dev(env, c["de"])
    dL, T = ops.gatv2_scores_bwd(rp, ci, de, L, R, a, H, negative_slope=SLOPE, want_T=True)
    assert np.array_equal(host(dL), c["dL"]) and np.array_equal(host(T), c["T"])
    empty = np.diff(P["rowptr"]) == 0
    assert not host(dL)[empty].view(np.uint32).any() and not host(T)[empty].view(np.uint32).any()   # an empty row writes +0
    only = ops.gatv2_scores_bwd(rp, ci, de, L, R, a, H, negative_slope=SLOPE)   # T = NULL
    assert torch.equal(only, dL)
    # beta = 1 onto a prefilled buffer, everything padded: NaN in the operands' pads, sentinels around both outputs, de with ldd > H
    Lw, Rw, dew = placed(env, c["L"], ld=F + 4)[0], placed(env, c["R"], ld=F + 8)[0], placed(env, c["de"], ld=H + 2)[0]
    out, obuf = placed(env, c["y0L"], ld=F + 12, fill=7.0)
    Tw, tbuf = placed(env, np.zeros((N_ROWS, F), dtype=np.float32), ld=F + 4, fill=5.0)
    before_o, before_t = host(obuf).copy(), host(tbuf).copy()
    ops.gatv2_scores_bwd(rp, ci, dew, Lw, Rw, a, H, negative_slope=SLOPE, out=out, beta=1.0, T_out=Tw)
    want1 = c["y0L"] + c["dL"]
    assert np.array_equal(host(out), want1) and np.array_equal(host(Tw), c["T"])
    assert np.array_equal(host(out)[empty], c["y0L"][empty])   # an empty row leaves dOwn unchanged
    check_margins(obuf, (N_ROWS, F), F + 12, 0, before_o)
    check_margins(tbuf, (N_ROWS, F), F + 4, 0, before_t)
    # the scalar path: a pointer one float off or an odd leading dimension, for each operand and output in turn
    av = placed(env, c["a"][None, :], offset=1)[0][0]
    for fail in ("own pointer", "other ld", "a pointer", "out ld", "T pointer"):
        own = placed(env, c["L"], offset=1 if fail == "own pointer" else 0)[0]
        other = placed(env, c["R"], ld=odd(F) if fail == "other ld" else None)[0]
        ldo, offt = (odd(F) if fail == "out ld" else F), (1 if fail == "T pointer" else 0)
        o, ob = placed(env, c["y0L"], ld=ldo, fill=7.0)
        t, tb = placed(env, np.zeros((N_ROWS, F), dtype=np.float32), offset=offt, fill=5.0)
        bo, bt = host(ob).copy(), host(tb).copy()
        ops.gatv2_scores_bwd(rp, ci, de, own, other, av if fail == "a pointer" else a, H, negative_slope=SLOPE, out=o, beta=1.0, T_out=t)
        assert np.array_equal(host(o), want1) and torch.equal(t, T), fail
        check_margins(ob, (N_ROWS, F), ldo, 0, bo)
        check_margins(tb, (N_ROWS, F), F, offt, bt)


@pytest.mark.parametrize("H,D", CELLS)
def test_backward_bits_on_the_transposed_pattern(env, P, H, D):
    """Own = R, Other = L, entry_map = map_t, beta = 1, T = NULL: equal to the restatement fed with de gathered by hand."""
    ops, torch, c, F = env["ops"], env["torch"], case(H, D), H * D
    L, R, a, de = dev(env, c["L"]), dev(env, c["R"]), dev(env, c["a"]), dev(env, c["de"])
    out = dev(env, c["y0R"]).clone()
    got = ops.gatv2_scores_bwd(P["rowptr_t_d"], P["colidx_t_d"], de, R, L, a, H, negative_slope=SLOPE, entry_map=P["map_t_d"], out=out, beta=1.0)
    assert got is out and np.array_equal(host(out), c["dR1"])
    # the gather done on the device by hand, no map: the same bits
    by_hand = ops.gatv2_scores_bwd(P["rowptr_t_d"], P["colidx_t_d"], de[P["map_t_d"].long()].contiguous(), R, L, a, H, negative_slope=SLOPE,
                                   out=dev(env, c["y0R"]).clone(), beta=1.0)
    assert torch.equal(by_hand, out)
    # misaligned, beta = 0, with T on this pattern too
    o, ob = placed(env, np.zeros((N_COLS, F), dtype=np.float32), ld=odd(F), offset=1, fill=7.0)
    bo = host(ob).copy()
    _, T = ops.gatv2_scores_bwd(P["rowptr_t_d"], P["colidx_t_d"], de, R, L, a, H, negative_slope=SLOPE, entry_map=P["map_t_d"], out=o, want_T=True)
    want0, wantT = gr.scores_bwd_ref(P["rowptr_t"], P["colidx_t"], c["de"], c["R"], c["L"], c["a"], H, SLOPE, entry_map=P["map_t"], want_T=True)
    assert np.array_equal(host(o), want0) and np.array_equal(host(T), wantT)
    check_margins(ob, (N_COLS, F), odd(F), 1, bo)


def test_l_is_r_on_a_square_pattern(env):
    ops = env["ops"]
    sq = pattern(320, 320)
    rp, ci = dev(env, sq["rowptr"]), dev(env, sq["colidx"])
    H, D = 4, 16
    rng = np.random.default_rng(3)
    Z = rng.uniform(-1, 1, (320, H * D)).astype(np.float32)
    a, de = rng.uniform(-1, 1, H * D).astype(np.float32), rng.uniform(-1, 1, (sq["nnz"], H)).astype(np.float32)
    Zd = dev(env, Z)
    got = ops.gatv2_scores(rp, ci, Zd, Zd, dev(env, a), H, negative_slope=SLOPE)
    assert np.array_equal(host(got), gr.scores_ref(sq["rowptr"], sq["colidx"], Z, Z, a, H, SLOPE))
    dZ, T = ops.gatv2_scores_bwd(rp, ci, dev(env, de), Zd, Zd, dev(env, a), H, negative_slope=SLOPE, want_T=True)
    want, wantT = gr.scores_bwd_ref(sq["rowptr"], sq["colidx"], de, Z, Z, a, H, SLOPE, want_T=True)
    assert np.array_equal(host(dZ), want) and np.array_equal(host(T), wantT)


@pytest.mark.parametrize("H,D", [(2, 3), (8, 8), (3, 64), (1, 260), (8, 260)])
def test_exact_family_equals_float64(env, P, H, D):
    """Every operation exact: out, dOwn, T, dR and colsum(T) carry the bits of the float64 results, whatever the order."""
    ops = env["ops"]
    c = gr.exact_case(7 * H + D, P["rowptr"], P["colidx"], N_COLS, H, D)
    L, R, a, de = (dev(env, c[k]) for k in ("L", "R", "a", "de"))
    slope = c["slope"]
    out = ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], L, R, a, H, negative_slope=slope)
    assert np.array_equal(host(out).astype(np.float64), gr.scores_ref64(P["rowptr"], P["colidx"], c["L"], c["R"], c["a"], H, slope))
    dL, T = ops.gatv2_scores_bwd(P["rowptr_d"], P["colidx_d"], de, L, R, a, H, negative_slope=slope, want_T=True)
    dL64, T64, da64 = gr.scores_bwd_ref64(P["rowptr"], P["colidx"], c["de"], c["L"], c["R"], c["a"], H, slope)
    assert np.array_equal(host(dL).astype(np.float64), dL64) and np.array_equal(host(T).astype(np.float64), T64)
    assert np.array_equal(host(ops.colsum(T)).astype(np.float64), da64)
    dR = ops.gatv2_scores_bwd(P["rowptr_t_d"], P["colidx_t_d"], de, R, L, a, H, negative_slope=slope, entry_map=P["map_t_d"])
    dR64, _, _ = gr.scores_bwd_ref64(P["rowptr_t"], P["colidx_t"], c["de"], c["R"], c["L"], c["a"], H, slope, entry_map=P["map_t"])
    assert np.array_equal(host(dR).astype(np.float64), dR64)
    assert np.abs(dL64).max() > 0 and np.abs(T64).max() > 0 and np.abs(da64).max() > 0


def test_a_pattern_without_entries(env):
    ops, torch = env["ops"], env["torch"]
    H, D, n = 2, 8, 5
    rp0 = torch.zeros(n + 1, dtype=torch.int32, device=env["dev"])
    ci0 = torch.zeros(0, dtype=torch.int32, device=env["dev"])
    Z = torch.ones((n, H * D), dtype=torch.float32, device=env["dev"])
    a = torch.ones(H * D, dtype=torch.float32, device=env["dev"])
    de = torch.zeros((0, H), dtype=torch.float32, device=env["dev"])
    assert tuple(ops.gatv2_scores(rp0, ci0, Z, Z, a, H).shape) == (0, H)
    out = torch.full((n, H * D), 3.0, dtype=torch.float32, device=env["dev"])
    ops.gatv2_scores_bwd(rp0, ci0, de, Z, Z, a, H, out=out, beta=1.0)
    assert (host(out) == 3.0).all()
    _, T = ops.gatv2_scores_bwd(rp0, ci0, de, Z, Z, a, H, out=out, want_T=True)
    assert not host(out).view(np.uint32).any() and not host(T).view(np.uint32).any()   # every row empty: +0


def test_argument_errors_come_back_without_a_launch(env, P):
    """Every refused call leaves its sentinel-filled outputs untouched and the device without an error."""
    capi, torch = env["capi"], env["torch"]
    lib = capi.lib()
    H, D = 2, 8
    F, c = H * D, case(2, 8)
    L, R, a, de = dev(env, c["L"]), dev(env, c["R"]), dev(env, c["a"]), dev(env, c["de"])
    out = torch.full((P["nnz"], H), 9.0, dtype=torch.float32, device=env["dev"])
    dOwn = torch.full((N_ROWS, F), 9.0, dtype=torch.float32, device=env["dev"])
    T = torch.full((N_ROWS, F), 9.0, dtype=torch.float32, device=env["dev"])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good_f = dict(n_rows=N_ROWS, n_cols=N_COLS, H=H, D=D, nnz=P["nnz"], rp=p(P["rowptr_d"]), ci=p(P["colidx_d"]), L=p(L), ldl=F, R=p(R), ldr=F,
                  a=p(a), slope=SLOPE, out=p(out), ldo=H)
    good_b = dict(n_rows=N_ROWS, n_cols=N_COLS, H=H, D=D, nnz=P["nnz"], rp=p(P["rowptr_d"]), ci=p(P["colidx_d"]), de=p(de), ldd=H, map=None,
                  own=p(L), ld_own=F, other=p(R), ld_other=F, a=p(a), slope=SLOPE, beta=0.0, dOwn=p(dOwn), ld_down=F, T=p(T), ldt=F)
    common = [dict(n_rows=-1), dict(n_cols=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(H=0), dict(D=0), dict(rp=None), dict(ci=None), dict(a=None)]
    bad_f = common + [dict(L=None), dict(R=None), dict(out=None), dict(ldl=F - 1), dict(ldr=F - 1), dict(ldo=H - 1)]
    bad_b = common + [dict(de=None), dict(own=None), dict(other=None), dict(dOwn=None), dict(ldd=H - 1), dict(ld_own=F - 1), dict(ld_other=F - 1),
                      dict(ld_down=F - 1), dict(ldt=F - 1), dict(beta=0.5)]
    for bad in bad_f:
        assert lib.gnnx_gatv2_scores_csr_f32(*{**good_f, **bad}.values(), None) == INVALID_ARG, bad
    for bad in bad_b:
        assert lib.gnnx_gatv2_scores_bwd_csr_f32(*{**good_b, **bad}.values(), None) == INVALID_ARG, bad
    torch.cuda.synchronize()
    assert (host(out) == 9.0).all() and (host(dOwn) == 9.0).all() and (host(T) == 9.0).all()
    # and the good argument lists are good
    assert lib.gnnx_gatv2_scores_csr_f32(*good_f.values(), None) == 0
    assert lib.gnnx_gatv2_scores_bwd_csr_f32(*good_b.values(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(out), c["out"]) and np.array_equal(host(dOwn), c["dL"]) and np.array_equal(host(T), c["T"])
    # the ops layer refuses shapes that do not fit before it calls
    ops = env["ops"]
    for call in (lambda: ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], L, R, a, 3),
                 lambda: ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], R, R, a, H),
                 lambda: ops.gatv2_scores(P["rowptr_d"], P["colidx_d"], L, R, a[:-1], H),
                 lambda: ops.gatv2_scores_bwd(P["rowptr_d"], P["colidx_d"], de[:, :1], L, R, a, H),
                 lambda: ops.gatv2_scores_bwd(P["rowptr_d"], P["colidx_d"], de, L, R, a, H, beta=1.0),
                 lambda: ops.gatv2_scores_bwd(P["rowptr_d"], P["colidx_d"], de, L, R, a, H, entry_map=P["map_t_d"].long())):
        with pytest.raises(capi.GnnxError):
            call()
