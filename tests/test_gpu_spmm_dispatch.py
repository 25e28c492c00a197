"""The aggregation's whole dispatch table held to an independent sum (run with -m gpu on an MI355X).

gnnx_spmm.hip's spmm_impl picks a kernel from the width and the alignment of the call: 16-byte pieces (VEC 4) or scalar lanes
(VEC 1), lane groups of 4 .. 64, the one-row-per-group kernel below G = 32 and the streaming kernel from there, one or several
feature tiles, and with a plan spmm_hub_kernel<VEC> and (VEC 4, f32 rows) the producer / consumer kernel -- each times seven modes,
each a separate instantiation.  Here every (VEC, G) cell, both edges of every G's range, several and ragged feature tiles, and the
scalar-lane fallback for a call that misses exactly one alignment condition meet tests/spmm_ref.py::spmm_ref -- float32 NumPy in
the header's order, pinned to the oracle and to float64 by tests/test_spmm_ref_cpu.py -- on one R-MAT graph with empty rows, every
short row length and hubs.  Every comparison is equality on every element (tests.golden_util.same: the sign of a zero is free).
The test id names the cell: the width, and for the unaligned cases the placement."""
import importlib

import numpy as np
import pytest

import oracle
from tests.golden_util import same
from tests.helpers import synth
from tests.spmm_ref import BF16_UNALIGNED_WIDTHS, UNALIGNED_WIDTHS, VEC1_WIDTHS, VEC4_WIDTHS, spmm_cell, spmm_ref

pytestmark = pytest.mark.gpu

N, E, SEED = 3001, 60000, 901
EPS = 1e-5
SENTINEL = 7.0
UNSUPPORTED = -7   # GNNX_ERR_UNSUPPORTED (include/gnnx.h)


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
def graph(env):
    """CSR(A) and CSR(A^T) of the one test graph on both sides, s / norm / the per-entry norm of the backward from the device."""
    ops = env["ops"]
    src, dst = synth.rmat_edges(SEED, N, E)
    rp, ci = oracle.coo_to_csr(src, dst, N)
    rT, cT = oracle.csr_transpose(rp, ci, N)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    assert np.array_equal(host(g.rowptr), rp) and np.array_equal(host(g.colidx), ci)
    assert np.array_equal(host(g.rowptr_t), rT) and np.array_equal(host(g.colidx_t), cT)
    for d in (np.diff(rp), np.diff(rT)):
        # empty rows, every length a lane group can meet below the streaming kernel's look-ahead, rows on either side of both plan
        # thresholds (16, 64) and of the producer / consumer cut (200), a row of several index chunks
        assert (d == 0).sum() >= 300 and set(range(38)) <= set(d.tolist())
        assert (d > 16).sum() >= 500 and (d > 64).sum() >= 100 and (d > 200).sum() >= 10 and d.max() >= 600
        assert ((d > 16) & (d <= 200)).sum() >= 400
    assert N % 64 and N % 32 and N % 16 and N % 8 and N % 4      # off every 256 / G and G / 2 grid
    g.norm_per_nz_t = ops.gather_rows(g.norm.reshape(-1, 1), g.colidx_t).reshape(-1)   # what ops.aggregate_bwd hands the kernel
    s, norm = host(g.s), host(g.norm)
    assert np.array_equal(host(g.norm_per_nz_t), norm[cT])
    vals = synth.uniform_pm1(930, (len(ci),))
    return dict(g=g, rp=rp, ci=ci, rT=rT, cT=cT, s=s, norm=norm, norm_nz_t=norm[cT], vals=vals, vals_d=dev(env, vals))


def make_inputs(env, F):
    ops = env["ops"]
    h = dict(H=synth.uniform_pm1(931, (N, F)), G=synth.uniform_pm1(932, (N, F)), bias=synth.uniform_pm1(933, (F,), scale=0.5),
             Y0=synth.uniform_pm1(934, (N, F)), gamma=synth.uniform_pm1(935, (F,)) + np.float32(1.5),
             beta=synth.uniform_pm1(936, (F,), scale=0.3))
    d = {k: dev(env, v) for k, v in h.items()}
    d["mean"], d["var"] = ops.bn_stats(d["H"])
    return h, d


# the prologue modes: name -> (BatchNorm, affine, ReLU) -- kernel modes 3 (ReLU), 4 (BatchNorm), 5 (BatchNorm + ReLU)
PROLOGUES = {"pro_relu": (False, False, True), "pro_bn": (True, False, False), "pro_bn_affine": (True, True, False),
             "pro_bn_relu": (True, False, True), "pro_bn_affine_relu": (True, True, True)}


def prologue_args(d, name):
    bn, affine, relu = PROLOGUES[name]
    stats = (d["mean"], d["var"]) if bn else (None, None)
    return stats + ((d["gamma"], d["beta"]) if affine else (None, None)), relu


def prologue_rows(env, d, name):
    """Host copy of the separate BatchNorm / ReLU kernel's output (pinned to the oracle by tests/test_gpu_parity.py): what the fused
    modes gather."""
    (mean, var, gamma, beta), relu = prologue_args(d, name)
    return host(env["ops"].bn_relu_fwd(d["H"], mean, var, gamma, beta, EPS, relu=relu))


def references(env, gr, h, d):
    rp, ci, rT, cT, s, norm = gr["rp"], gr["ci"], gr["rT"], gr["cT"], gr["s"], gr["norm"]
    H, G, bias, Y0 = h["H"], h["G"], h["bias"], h["Y0"]
    r = {"fwd": spmm_ref(rp, ci, H, rowscale=norm, bias=bias),
         "fwd_relu": spmm_ref(rp, ci, H, rowscale=norm, bias=bias, relu_out=True),
         "fwd_acc": spmm_ref(rp, ci, H, rowscale=norm, bias=bias, y0=Y0),
         "fwd_acc_relu": spmm_ref(rp, ci, H, rowscale=norm, bias=bias, y0=Y0, relu_out=True),
         "bwd_norm": spmm_ref(rT, cT, G, vals=gr["norm_nz_t"]),
         "vals": spmm_ref(rp, ci, H, vals=gr["vals"]),
         "sym": spmm_ref(rp, ci, H, colscale=s, rowscale=s, bias=bias),
         "sym_t": spmm_ref(rT, cT, G, colscale=s, rowscale=s, bias=bias),
         "vals_sym": spmm_ref(rp, ci, H, vals=gr["vals"], colscale=s, rowscale=norm)}
    for name in PROLOGUES:
        r[name] = spmm_ref(rp, ci, prologue_rows(env, d, name), rowscale=norm, bias=bias)
    return r


def run_modes(env, gr, d, use_plan):
    ops, g = env["ops"], gr["g"]
    plan, plan_t = (g.plan, g.plan_t) if use_plan else (None, None)
    H, G, bias = d["H"], d["G"], d["bias"]
    out = {"fwd": ops.aggregate_fwd(g, H, bias, use_plan=use_plan),
           "fwd_relu": ops.aggregate_fwd(g, H, bias, relu_out=True, use_plan=use_plan),
           "fwd_acc": ops.spmm(g.rowptr, g.colidx, H, out=d["Y0"].clone(), rowscale=g.norm, bias=bias, beta=1.0, plan=plan),
           "fwd_acc_relu": ops.spmm(g.rowptr, g.colidx, H, out=d["Y0"].clone(), rowscale=g.norm, bias=bias, beta=1.0, plan=plan,
                                    relu_out=True),
           "bwd_norm": ops.aggregate_bwd(g, G, use_plan=use_plan),
           "vals": ops.spmm(g.rowptr, g.colidx, H, vals=gr["vals_d"], plan=plan),
           "sym": ops.aggregate_fwd_sym(g, H, bias, use_plan=use_plan),
           "sym_t": ops.spmm(g.rowptr_t, g.colidx_t, G, colscale=g.s, rowscale=g.s, bias=bias, plan=plan_t),
           "vals_sym": ops.spmm(g.rowptr, g.colidx, H, vals=gr["vals_d"], colscale=g.s, rowscale=g.norm, plan=plan)}
    for name in PROLOGUES:
        (mean, var, gamma, beta), relu = prologue_args(d, name)
        bn = (mean, var, gamma, beta, EPS) if mean is not None else None
        out[name] = ops.aggregate_fwd(g, H, bias, bn=bn, relu_in=relu, use_plan=use_plan)
    return out


def differences(got, ref):
    """'' when got == ref everywhere, else how many elements differ and where the first one sits."""
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    ne = ~(got == ref)
    if not ne.any():
        return ""
    r, c = np.argwhere(ne)[0]
    return f"{int(ne.sum())} of {ne.size} elements in {int(ne.any(1).sum())} rows differ, first at [{r}, {c}]: {got[r, c]!r} != {ref[r, c]!r}"


def plan_configs(F):
    cfgs = [("no plan", None), ("chunk 64", dict(chunk=64, max_feat=F)), ("chunk 16, big rows > 200", dict(chunk=16, max_feat=F, big_rows=200))]
    if F % 4 == 0:
        cfgs.append(("chunk 16, every hub row big", dict(chunk=16, max_feat=F, big_rows=0)))
    return cfgs


@pytest.mark.parametrize("F", VEC4_WIDTHS + VEC1_WIDTHS, ids=lambda F: "F{}-vec{}-G{}-{}-tiles{}".format(F, *spmm_cell(F)))
def test_aligned_rows_every_mode_and_plan_equal_the_restated_sum(env, graph, F):
    """Aligned f32 rows: mode 0 with rowscale + bias (beta 0 / 1, with and without the ReLU epilogue), mode 2 (the backward's
    per-entry norm on CSR(A^T), random values on CSR(A)), mode 1 on both CSRs, mode 6, and the three prologue modes with and without
    gamma / beta -- unplanned, with hub rows on spmm_hub_kernel and plan blocks (chunk 64), with both hub kernels (chunk 16, rows
    above 200 on the producer / consumer kernel where the rows are 16-byte pieces) and, for those widths, with every hub row on it."""
    g = graph["g"]
    h, d = make_inputs(env, F)
    ref = references(env, graph, h, d)
    bad = []
    for what, cfg in plan_configs(F):
        if cfg is not None:
            plan, plan_t = g.make_plans(**cfg)
            assert plan.n_split_rows > 0 and plan_t.n_split_rows > 0, "the plan is meant to have hub rows"
        got = run_modes(env, graph, d, use_plan=cfg is not None)
        assert set(got) == set(ref)
        for name in ref:
            diff = differences(host(got[name]), ref[name])
            if diff:
                bad.append(f"{what} / {name}: {diff}")
    g.plan = g.plan_t = None
    assert not bad, f"F = {F} {spmm_cell(F)}:\n  " + "\n  ".join(bad)


# ---- the scalar-lane fallback: widths that are multiples of 4 in a call that misses exactly one vec4 condition -------------------
def place_matrix(env, t, how):
    """A view holding t inside a sentinel-filled buffer: 'off1' = columns 1 .. F of an (n, F + 5) buffer (4-byte aligned base, odd
    pitch), 'ld' = the first F columns of an (n, F + 2) buffer (aligned base, a pitch that is no multiple of 4).  -> (view, buffer)"""
    torch = env["torch"]
    n, F = t.shape
    buf = torch.full((n, F + 5 if how == "off1" else F + 2), SENTINEL, dtype=t.dtype, device=t.device)
    view = buf[:, 1:1 + F] if how == "off1" else buf[:, :F]
    view.copy_(t)
    return view, buf


def place_vector(env, t):
    buf = env["torch"].full((t.numel() + 5,), SENTINEL, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()]
    view.copy_(t)
    return view


def untouched_outside(env, view, buf):
    """every element of buf outside the view still holds the sentinel"""
    torch = env["torch"]
    mask = torch.ones_like(buf, dtype=torch.bool)
    c0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    mask[:, c0:c0 + view.shape[1]] = False
    return bool((buf[mask] == SENTINEL).all())


PLACEMENTS = ("x_off1", "y_off1", "bias_off1", "x_ld", "y_ld", "mean_off1", "gamma_off1")
FALLBACK_MODES = ("fwd", "bwd_norm", "sym", "pro_bn_affine_relu")   # kernel modes 0, 2, 1 and 5


@pytest.fixture(scope="module")
def fallback_case(env, graph):
    """inputs and the four references of a width, computed once for all its placements"""
    cache = {}

    def get(F):
        if F not in cache:
            h, d = make_inputs(env, F)
            rp, ci, rT, cT, s, norm, bias = graph["rp"], graph["ci"], graph["rT"], graph["cT"], graph["s"], graph["norm"], h["bias"]
            ref = {"fwd": spmm_ref(rp, ci, h["H"], rowscale=norm, bias=bias),
                   "bwd_norm": spmm_ref(rT, cT, h["H"], vals=graph["norm_nz_t"], bias=bias),
                   "sym": spmm_ref(rp, ci, h["H"], colscale=s, rowscale=s, bias=bias),
                   "pro_bn_affine_relu": spmm_ref(rp, ci, prologue_rows(env, d, "pro_bn_affine_relu"), rowscale=norm, bias=bias)}
            cache[F] = (d, ref)
        return cache[F]
    return get


def run_fallback_mode(env, gr, mode, X, Y, bias, stats, use_plan):
    ops, g = env["ops"], gr["g"]
    plan, plan_t = (g.plan, g.plan_t) if use_plan else (None, None)
    if mode == "fwd":
        return ops.spmm(g.rowptr, g.colidx, X, out=Y, rowscale=g.norm, bias=bias, plan=plan)
    if mode == "bwd_norm":
        return ops.spmm(g.rowptr_t, g.colidx_t, X, out=Y, vals=g.norm_per_nz_t, bias=bias, plan=plan_t)
    if mode == "sym":
        return ops.spmm(g.rowptr, g.colidx, X, out=Y, colscale=g.s, rowscale=g.s, bias=bias, plan=plan)
    return ops.spmm(g.rowptr, g.colidx, X, out=Y, rowscale=g.norm, bias=bias, plan=plan, bn=stats + (EPS,), relu_in=True)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("F", UNALIGNED_WIDTHS, ids=lambda F: "F{}-vec{}-G{}-{}-tiles{}".format(F, *spmm_cell(F, aligned=False)))
def test_unaligned_call_takes_the_scalar_lanes_and_keeps_the_bits(env, graph, fallback_case, F, placement):
    """One vec4 condition fails at a time -- X, Y or the bias 4 bytes off a 16-byte boundary, a leading dimension that is no multiple
    of 4, a prologue vector 4 bytes off: the header states no alignment precondition, the call must fall back to the scalar lanes
    (spmm_hub_kernel<1> for the plan's hub rows) and give the restated sum and the aligned call's bits, and store nothing outside Y."""
    torch, g = env["torch"], graph["g"]
    d, ref = fallback_case(F)
    modes = ("pro_bn_affine_relu",) if placement in ("mean_off1", "gamma_off1") else FALLBACK_MODES
    stats = (d["mean"], d["var"], d["gamma"], d["beta"])
    bad = []
    for what, cfg in plan_configs(F)[:2]:   # unplanned, and hub rows + plan blocks (chunk 64)
        if cfg is not None:
            plan, plan_t = g.make_plans(**cfg)
            assert plan.n_split_rows > 0 and plan_t.n_split_rows > 0
        for mode in modes:
            aligned = run_fallback_mode(env, graph, mode, d["H"], None, d["bias"], stats, cfg is not None)
            X, Y, ybuf, bias, st = d["H"], None, None, d["bias"], stats
            if placement in ("x_off1", "x_ld"):
                X, _ = place_matrix(env, d["H"], placement[2:])
            elif placement in ("y_off1", "y_ld"):
                Y, ybuf = place_matrix(env, torch.full((N, F), SENTINEL, dtype=torch.float32, device=env["dev"]), placement[2:])
            elif placement == "bias_off1":
                bias = place_vector(env, d["bias"])
            elif placement == "mean_off1":
                st = (place_vector(env, d["mean"]),) + stats[1:]
            else:
                st = stats[:2] + (place_vector(env, d["gamma"]),) + stats[3:]
            moved = [t for t in (X, Y, bias, st[0], st[2]) if t is not None and (t.data_ptr() % 16 or (t.dim() == 2 and t.stride(0) % 4))]
            assert len(moved) == 1, "exactly one operand is meant to miss the vec4 conditions"
            got = run_fallback_mode(env, graph, mode, X, Y, bias, st, cfg is not None)
            diff = differences(host(got), ref[mode])
            if diff:
                bad.append(f"{what} / {mode} vs the restated sum: {diff}")
            if not torch.equal(got, aligned):
                bad.append(f"{what} / {mode}: differs from the aligned call")
            if ybuf is not None and not untouched_outside(env, Y, ybuf):
                bad.append(f"{what} / {mode}: stored outside Y")
    g.plan = g.plan_t = None
    assert not bad, f"F = {F}, {placement}:\n  " + "\n  ".join(bad)


# ---- bf16 rows that are not 8-byte aligned ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [1, 2], ids=["off1-pitch-odd", "off2-pitch-mult4"])
@pytest.mark.parametrize("F", BF16_UNALIGNED_WIDTHS, ids=lambda F: "F{}-vec{}-G{}-{}-tiles{}".format(F, *spmm_cell(F, aligned=False)))
def test_bf16_rows_off_the_8_byte_grid(env, graph, F, offset):
    """bf16 feature rows as a view at column 1 (2-byte aligned, odd pitch) or 2 (4-byte aligned, a pitch of whole 8-byte pieces) of a
    wider buffer: the scalar-lane kernels with 2-byte loads, the plan's hub rows handed back to the row / streaming kernel.  The
    result is the restated sum over the widened rows and the aligned bf16 call's bits (modes 0, 2, 1, 6; unplanned and chunk 64)."""
    ops, torch, g = env["ops"], env["torch"], graph["g"]
    h, d = make_inputs(env, F)
    Xb = ops.to_bf16(d["H"])
    Xw = host(Xb.float())
    assert not np.array_equal(Xw, h["H"]) and np.array_equal(Xw.view(np.uint32) & 0xffff, np.zeros_like(Xw, dtype=np.uint32))
    buf = torch.zeros((N, F + (5 if offset == 1 else 4)), dtype=torch.bfloat16, device=env["dev"])
    Xv = buf[:, offset:offset + F]
    Xv.copy_(Xb)
    assert Xv.data_ptr() % 8 == 2 * offset and Xb.data_ptr() % 8 == 0 and (offset == 1 or Xv.stride(0) % 4 == 0)
    rp, ci, rT, cT, s, norm = graph["rp"], graph["ci"], graph["rT"], graph["cT"], graph["s"], graph["norm"]
    ref = {"fwd": spmm_ref(rp, ci, Xw, rowscale=norm, bias=h["bias"]),
           "bwd_norm": spmm_ref(rT, cT, Xw, vals=graph["norm_nz_t"]),
           "sym": spmm_ref(rp, ci, Xw, colscale=s, rowscale=s, bias=h["bias"]),
           "vals_sym": spmm_ref(rp, ci, Xw, vals=graph["vals"], colscale=s, rowscale=norm)}

    def run(X, use_plan):
        plan, plan_t = (g.plan, g.plan_t) if use_plan else (None, None)
        return {"fwd": ops.spmm(g.rowptr, g.colidx, X, rowscale=g.norm, bias=d["bias"], plan=plan),
                "bwd_norm": ops.spmm(g.rowptr_t, g.colidx_t, X, vals=g.norm_per_nz_t, plan=plan_t),
                "sym": ops.spmm(g.rowptr, g.colidx, X, colscale=g.s, rowscale=g.s, bias=d["bias"], plan=plan),
                "vals_sym": ops.spmm(g.rowptr, g.colidx, X, vals=graph["vals_d"], colscale=g.s, rowscale=g.norm, plan=plan)}
    bad = []
    for what, cfg in plan_configs(F)[:2]:
        if cfg is not None:
            plan, plan_t = g.make_plans(**cfg)
            assert plan.n_split_rows > 0 and plan_t.n_split_rows > 0
        got, aligned = run(Xv, cfg is not None), run(Xb, cfg is not None)
        for name in ref:
            diff = differences(host(got[name]), ref[name])
            if diff:
                bad.append(f"{what} / {name} vs the restated sum: {diff}")
            if not torch.equal(got[name], aligned[name]):
                bad.append(f"{what} / {name}: differs from the aligned bf16 call")
    g.plan = g.plan_t = None
    assert not bad, f"F = {F}, column offset {offset}:\n  " + "\n  ".join(bad)


def test_backward_with_batchnorm_sums_refuses_unaligned_rows(env, graph):
    """gnnx_spmm_csr_bn_sums_f32 covers 16-byte aligned rows only and says so: GNNX_ERR_UNSUPPORTED for a G that is 4 bytes off, where
    the same call on the aligned G is accepted."""
    ops, capi, g = env["ops"], env["capi"], graph["g"]
    h, d = make_inputs(env, 128)
    dY, _, _ = ops.aggregate_bwd_bn_sums(g, d["G"], d["H"], d["mean"], d["var"], d["gamma"], d["beta"], EPS, True, use_plan=False)
    assert same(host(dY), spmm_ref(graph["rT"], graph["cT"], h["G"], vals=graph["norm_nz_t"]))
    Gv, _ = place_matrix(env, d["G"], "off1")
    with pytest.raises(capi.GnnxError) as err:
        ops.aggregate_bwd_bn_sums(g, Gv, d["H"], d["mean"], d["var"], d["gamma"], d["beta"], EPS, True, use_plan=False)
    assert err.value.status == UNSUPPORTED
