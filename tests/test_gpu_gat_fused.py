"""GPU tests of the fused graph-attention calls (run with -m gpu on an MI355X): ops.gat_aggregate / gat_aggregate_bwd_rows /
gat_aggregate_bwd_cols and GatStack(fused=True) against tests/gat_fused_ref.py (float32 up to the argument of exp, float64 from there).

Bars are derived, |got - ref| <= c * 2^-24 * S per output element, S the float64 sum of the absolute terms of the element and c the
rounded operations on its longest chain (+ 4 for expf); tests/gat_fused_ref.py derives each c next to its function.  rowmax compares
equal.  Pattern A is tests/edge_softmax_ref.py pattern_a: 16 384 columns, rows of 0 .. 12 293 entries on every boundary (one segment |
two, a short fourth segment) between runs of short and empty rows.  Each test prints the worst fraction of its bar."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import gat_fused_ref as gr
from tests import sddmm_ref as sr
from tests.helpers import synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64), (8, 8), (2, 64), (4, 6), (1, 260)]   # (4, 6): scalar loads; (1, 260): a second chunk per lane
SLOPE = 0.2
U = 2.0 ** -24


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
def pat(env):
    rp, ci, _ = er.pattern_a()
    rp_t, ci_t = sr.transpose_csr(rp, ci, er.N_COLS_A)   # A is the transposed pattern of this one
    return dict(rp=rp, ci=ci, rp_t=rp_t, ci_t=ci_t, n=len(rp) - 1, nc=er.N_COLS_A, d=np.diff(rp), rp_d=dev(env, rp), ci_d=dev(env, ci))


def operands(pat, H, D, epilogue, n_rows, n_cols):
    """float32 operands of a pattern with n_rows rows and n_cols columns; epilogue: bias and ReLU on"""
    rng = np.random.default_rng(1000 * H + D)
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return dict(X=f(n_cols, H * D), rowterm=f(n_rows, H) * 2, colterm=f(n_cols, H) * 2, G=f(n_rows, H * D),
                bias=f(H * D) if epilogue else None)


def held(got, ref, c, S, what):
    """|got - ref| <= c * 2^-24 * S, element by element; prints the worst fraction of the bar"""
    err, bar = np.abs(got.astype(np.float64) - ref), np.broadcast_to(c, ref.shape) * U * S
    frac = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))))
    print(f"{what}: worst |err| / bar = {frac:.4f}")
    assert frac <= 1.0, what


def per_feature(c, n):
    return np.asarray(c, dtype=np.float64).reshape(n, 1)


@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("H,D,offset", [(h, d, False) for h, d in SHAPES] + [(8, 8, True)])
def test_forward(env, pat, H, D, offset, epilogue):
    ops, torch = env["ops"], env["torch"]
    o = operands(pat, H, D, epilogue, pat["n"], pat["nc"])
    ref = gr.forward(pat["rp"], pat["ci"], o["X"], H, o["rowterm"], o["colterm"], SLOPE, o["bias"], epilogue)
    X = dev(env, o["X"])
    if offset:   # ldx > F and a base 4 bytes off alignment, between NaN pads: the scalar-load path
        buf = torch.full((pat["nc"] * (H * D + 3) + 1,), float("nan"), device=env["dev"])
        X = buf[1:].view(pat["nc"], H * D + 3)[:, :H * D]
        X.copy_(dev(env, o["X"]))
        assert X.data_ptr() % 16 == 4
    Y, m, z = ops.gat_aggregate(pat["rp_d"], pat["ci_d"], X, H, dev(env, o["rowterm"]), dev(env, o["colterm"]), SLOPE,
                                bias=None if o["bias"] is None else dev(env, o["bias"]), relu_out=epilogue)
    Y, m, z = host(Y), host(m), host(z)
    assert np.array_equal(m, ref["rowmax"])
    d = pat["d"]
    held(z, ref["rowsum"], per_feature(gr.c_rowsum(d), pat["n"]), ref["rowsum"], "rowsum")
    held(Y, ref["Y"], per_feature(gr.c_Y(d), pat["n"]), ref["S_Y"], "Y")
    empty = d == 0
    act = np.zeros(H * D, np.float32) if o["bias"] is None else (np.maximum(o["bias"], 0) if epilogue else o["bias"])
    assert np.all(np.isneginf(m[empty])) and np.all(z[empty] == 0) and not np.signbit(z[empty]).any()
    assert np.array_equal(Y[empty], np.broadcast_to(act, (int(empty.sum()), H * D)))


@pytest.mark.parametrize("epilogue,beta", [(False, 0.0), (True, 1.0)], ids=["plain_beta0", "bias_relu_beta1"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_backward(env, pat, H, D, epilogue, beta):
    ops = env["ops"]
    n, nc, d = pat["n"], pat["nc"], pat["d"]
    # row side: A is the forward pattern; Y, rowmax, rowsum are the float32 roundings of the reference forward
    o = operands(pat, H, D, epilogue, n, nc)
    fw = gr.forward(pat["rp"], pat["ci"], o["X"], H, o["rowterm"], o["colterm"], SLOPE, o["bias"], epilogue)
    Y, z = fw["Y"].astype(np.float32), fw["rowsum"].astype(np.float32)
    G = np.where(Y > 0, o["G"], 0).astype(np.float32) if epilogue else o["G"]   # the caller applies the ReLU mask
    ref = gr.backward(pat["rp"], pat["ci"], H, SLOPE, G, o["X"], Y, o["bias"], o["rowterm"], o["colterm"], fw["rowmax"], z)
    drow, dot = ops.gat_aggregate_bwd_rows(pat["rp_d"], pat["ci_d"], dev(env, G), dev(env, o["X"]), dev(env, Y), H, dev(env, o["rowterm"]),
                                           dev(env, o["colterm"]), dev(env, fw["rowmax"]), dev(env, z), SLOPE,
                                           bias=None if o["bias"] is None else dev(env, o["bias"]))
    held(host(dot), ref["dot"], gr.c_dot(D), ref["S_dot"], "dot")
    held(host(drow), ref["drowterm"], per_feature(gr.c_dterm(d, D), n), ref["S_drowterm"], "drowterm")
    assert np.all(host(drow)[d == 0] == 0)

    # column side: A is the TRANSPOSED pattern (row c of A, entries i < 16 384), so its hub rows are this call's hub rows; the
    # forward pattern is A^T, whose rows i own G, rowterm, rowmax, rowsum and dot
    o = operands(pat, H, D, epilogue, nc, n)
    fw = gr.forward(pat["rp_t"], pat["ci_t"], o["X"], H, o["rowterm"], o["colterm"], SLOPE, None, False)
    z = np.where(np.diff(pat["rp_t"])[:, None] > 0, fw["rowsum"], 1).astype(np.float32)
    dot = np.random.default_rng(D).uniform(-1, 1, (nc, H)).astype(np.float32)
    ref = gr.backward(pat["rp_t"], pat["ci_t"], H, SLOPE, o["G"], o["X"], None, None, o["rowterm"], o["colterm"], fw["rowmax"], z, dot=dot)
    old = np.random.default_rng(H).uniform(-1, 1, (n, H * D)).astype(np.float32)
    dX, dcol = ops.gat_aggregate_bwd_cols(pat["rp_d"], pat["ci_d"], dev(env, o["G"]), dev(env, o["X"]), H, dev(env, o["rowterm"]),
                                          dev(env, o["colterm"]), dev(env, fw["rowmax"]), dev(env, z), dev(env, dot), SLOPE,
                                          out=dev(env, old), beta=beta)
    held(host(dX), ref["dX"] + beta * old, per_feature(gr.c_dX(d), n), ref["S_dX"] + beta * np.abs(old), "dX")
    held(host(dcol), ref["dcolterm"], per_feature(gr.c_dterm(d, D), n), ref["S_dcolterm"], "dcolterm")


def test_two_runs_give_the_same_bits(env, pat):
    ops, torch, (H, D) = env["ops"], env["torch"], (8, 8)
    o = {k: None if v is None else dev(env, v) for k, v in operands(pat, H, D, True, pat["n"], pat["nc"]).items()}
    t = {k: dev(env, v) for k, v in operands(pat, H, D, False, pat["nc"], pat["n"]).items() if v is not None}
    runs = []
    for _ in range(2):
        Y, m, z = ops.gat_aggregate(pat["rp_d"], pat["ci_d"], o["X"], H, o["rowterm"], o["colterm"], SLOPE, bias=o["bias"], relu_out=True)
        drow, dot = ops.gat_aggregate_bwd_rows(pat["rp_d"], pat["ci_d"], o["G"], o["X"], Y, H, o["rowterm"], o["colterm"], m, z, SLOPE, bias=o["bias"])
        stat = torch.ones((pat["nc"], H), device=env["dev"])
        dX, dcol = ops.gat_aggregate_bwd_cols(pat["rp_d"], pat["ci_d"], t["G"], t["X"], H, t["rowterm"], t["colterm"], stat * 5, stat, stat, SLOPE)
        runs.append((Y, m, z, drow, dot, dX, dcol))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- GatStack(fused=True) ------------------------------------------------------------------------------------------------------------
N, E, DIMS = 1 << 10, 8000, [32, 32, 8]


def model64(torch, rowptr, colidx, X, params, heads, rows, target):
    """The GAT of GatStack in float64 autograd (A as the stack's [2 Hh, F] matrix) and the loss kernel's form of the cross entropy."""
    rows_e, cols_e = torch.from_numpy(er.row_of_entries(rowptr)), torch.from_numpy(colidx.astype(np.int64))
    h, L = torch.from_numpy(X.astype(np.float64)), len(heads)
    for l, Hh in enumerate(heads):
        H = h @ params["W"][l].T
        ER = H @ params["A"][l].T
        e = torch.nn.functional.leaky_relu(ER[rows_e, :Hh] + ER[cols_e, Hh:], float(np.float32(SLOPE)))
        m = torch.full((N, Hh), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, Hh), e.detach(), "amax")
        x = torch.exp(e - m[rows_e])
        alpha = x / torch.zeros((N, Hh), dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        Y = torch.zeros_like(H).index_add(0, rows_e, alpha.repeat_interleave(H.shape[1] // Hh, 1) * H[cols_e]) + params["b"][l]
        h = torch.relu(Y) if l + 1 < L else Y
    z = h[torch.from_numpy(rows.astype(np.int64))]
    picked = z[torch.arange(len(rows)), torch.from_numpy(target.astype(np.int64))[rows]]
    return h, (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(rows)


@pytest.mark.parametrize("heads", [[4, 1], None], ids=["heads_4_1", "one_head"])
@pytest.mark.parametrize("diagonal", [False, True], ids=["stripped", "filled"])
def test_stack_step_vs_float64(env, diagonal, heads):
    """One training step (lr = 0) against float64 autograd at the bars of tests/test_gpu_gat.py::test_one_step_vs_float64 -- 1e-5 *
    max(1, |ref|) for the loss, 2e-5 * max(|ref|_max, 1e-3) for every gradient -- and, at the gradient bar, the logits against float64
    and against the fused=False stack of the same seed."""
    ops, torch = env["ops"], env["torch"]
    src, dst = synth.rmat_edges(91, N, E)
    s, d = dev(env, src), dev(env, dst)
    if diagonal:
        w = torch.ones(s.numel(), dtype=torch.float32, device=env["dev"])
        rp, ci, _ = ops.csr_from_coo_weighted(s, d, w, N, ops.DIAG_FILL)
        rp_t, ci_t, _ = ops.csr_from_coo_weighted(d, s, w, N, ops.DIAG_FILL)
        g = ops.CsrGraph(N, rp, ci, rp_t, ci_t)
    else:
        g = ops.CsrGraph.from_coo(s, d, N)
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target, rows = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32), np.arange(0, N, 3, dtype=np.int32)
    net = ops.GatStack(g, DIMS, seed=950, heads=heads, fused=True)
    assert net.map_t is None and getattr(g, "_map_t", None) is None   # no transpose map on the fused path
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    params = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in ("W", "A", "b")}
    loss = net.train_step(dev(env, X), dev(env, target), dev(env, rows), lr=0.0)
    logits = host(net.forward(dev(env, X)))
    logits_ref, ref = model64(torch, host(g.rowptr), host(g.colidx), X, params, net.heads, rows, target)
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    close = lambda got, r: np.abs(got - r).max() <= 2e-5 * max(np.abs(r).max(), 1e-3)  # noqa: E731
    for l in range(len(net.W)):
        mask = host(net.A_mask[l])
        for got, r, nm in ((net.dW[l], params["W"][l].grad.numpy(), "dW"), (net.dA[l], params["A"][l].grad.numpy() * mask, "dA"),
                           (net.db[l], params["b"][l].grad.numpy(), "db")):
            assert np.abs(r).max() > 0 and close(host(got), r), f"{nm}{l}"
    assert close(logits, logits_ref.detach().numpy())
    plain = ops.GatStack(g, DIMS, seed=950, heads=heads)
    for l in range(len(DIMS) - 1):
        plain.b[l].copy_(net.b[l])
    assert close(host(plain.forward(dev(env, X))), logits)


def test_relabelled_graph(env):
    """The fused stack on a relabelled graph (rows in original-id order, which the transpose map refuses): one step gives, through g.nid,
    the logits and gradients of the same stack on the plain graph, at the bars of test_stack_step_vs_float64."""
    ops = env["ops"]
    src, dst = synth.rmat_edges(91, N, E)
    X, target = dev(env, synth.uniform_pm1(93, (N, DIMS[0]))), dev(env, ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32))
    rows = dev(env, np.arange(0, N, 3, dtype=np.int32))
    out = []
    for relabel in (None, "scramble"):
        g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N, relabel=relabel)
        net = ops.GatStack(g, DIMS, seed=950, heads=[4, 1], fused=True)
        r = rows if relabel is None else g.nid[rows.long()].contiguous()
        loss = net.train_step(g.to_new_order(X), g.to_new_order(target), r, lr=0.0)
        out.append([host(loss), host(g.to_vertex_order(net.forward(g.to_new_order(X))))] + [host(t) for t in net.grads()])
    assert out[1][0] == pytest.approx(out[0][0], rel=1e-5)
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.abs(a - b).max() <= 2e-5 * max(np.abs(a).max(), 1e-3)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
FWD, ROWS, COLS = "gnnx_gat_aggregate_csr_f32", "gnnx_gat_aggregate_bwd_rows_csr_f32", "gnnx_gat_aggregate_bwd_cols_csr_f32"
REFUSALS = [(FWD, dict(D=513), -7), (FWD, dict(H=65536, D=256), -7), (FWD, dict(H=0), -1), (FWD, dict(D=0), -1), (FWD, dict(nnz=2 ** 31), -1),
            (FWD, dict(n_rows=-1), -1), (FWD, dict(rs=1), -1), (FWD, dict(ldx=15), -1), (FWD, dict(ldy=15), -1), (FWD, dict(null="colterm"), -1),
            (FWD, dict(null="X"), -1), (FWD, dict(null="Y"), -1), (FWD, dict(ws_bytes=64), -4), (FWD, dict(null="ws"), -4),
            (ROWS, dict(ldg=15), -1), (ROWS, dict(ds=1), -1), (ROWS, dict(null="rowmax"), -1), (ROWS, dict(null="dot"), -1),
            (ROWS, dict(D=513), -7), (ROWS, dict(ws_bytes=64), -4),
            (COLS, dict(beta=2.0), -1), (COLS, dict(ldy=15), -1), (COLS, dict(ds=1), -1), (COLS, dict(null="rowsum"), -1),
            (COLS, dict(null="Y"), -1), (COLS, dict(H=0), -1), (COLS, dict(H=65536, D=256), -7), (COLS, dict(null="ws"), -4)]


@pytest.mark.parametrize("call,change,status", REFUSALS, ids=[f"{c[19:-8] or 'fwd'}-" + "_".join(f"{a}_{b}" for a, b in k.items()) for c, k, _ in REFUSALS])
def test_refusals_write_nothing(env, pat, call, change, status):
    """Every status the header lists, on each of the three calls (valid arguments of (H, D) = (2, 8) on pattern A with one change; Y
    stands for the call's [rows, F] output, ds for its term-gradient stride): the call returns it and every sentinel-filled array,
    outputs included, keeps its bits.  Nothing is read either, so the arrays need not have the size a refused (H, D) would ask for."""
    torch, L = env["torch"], env["capi"].lib()
    v = dict(n_rows=pat["n"], nnz=len(pat["ci"]), H=2, D=8, rs=2, ds=2, ldx=16, ldy=16, ldg=16, beta=0.0, null=None, ws_bytes=1 << 22)
    v.update(change)
    if v["H"] > 2:   # the passes limit: consistent strides, so that only the limit refuses
        v.update(rs=v["H"], ds=v["H"], ldx=v["H"] * v["D"], ldy=v["H"] * v["D"], ldg=v["H"] * v["D"])
    t = {k: torch.full((pat["nc"], 16), 7.0, device=env["dev"]) for k in ("rowterm", "colterm", "X", "G", "Yin", "Y", "rowmax", "rowsum", "dot", "dterm")}
    t["ws"] = torch.full((1 << 20,), 7.0, device=env["dev"])
    P = lambda k: None if v["null"] == k else C.c_void_p(t[k].data_ptr())  # noqa: E731
    head = [v["n_rows"], pat["nc"], v["nnz"], C.c_void_p(pat["rp_d"].data_ptr()), C.c_void_p(pat["ci_d"].data_ptr()), v["H"], v["D"], P("rowterm"),
            v["rs"], P("colterm"), v["rs"], SLOPE]
    tail = [P("ws"), v["ws_bytes"], None]
    if call == FWD:
        rc = getattr(L, call)(*head, P("X"), v["ldx"], None, 1, P("Y"), v["ldy"], P("rowmax"), P("rowsum"), *tail)
    elif call == ROWS:
        rc = getattr(L, call)(*head, P("G"), v["ldg"], P("X"), v["ldx"], P("Yin"), 16, None, P("rowmax"), P("rowsum"), P("dterm"), v["ds"], P("dot"), *tail)
    else:
        rc = getattr(L, call)(*head, P("G"), v["ldg"], P("X"), v["ldx"], P("rowmax"), P("rowsum"), P("dot"), v["beta"], P("Y"), v["ldy"], P("dterm"),
                              v["ds"], *tail)
    torch.cuda.synchronize()
    assert rc == status
    assert all(bool((a == 7.0).all()) for a in t.values())
