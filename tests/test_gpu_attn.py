"""GPU tests of the dot-product attention calls (run with -m gpu on an MI355X): ops.attn_aggregate / attn_aggregate_bwd_rows /
attn_aggregate_bwd_cols and TransformerStack against tests/attn_ref.py (float64 NumPy from the float32 operands on).

Bars are derived, |got - ref| <= c * 2^-24 * S per output element; tests/attn_ref.py derives S and c next to each function.  Pattern A
is tests/edge_softmax_ref.py pattern_a: 16 384 columns, rows of 0 .. 12 293 entries on every boundary (one segment | two, a short
fourth segment) between runs of short and empty rows; eidx is a fixed permutation of the entries.  Each test prints the worst fraction
of its bar.  Observed on an MI355X (worst over all cases): rowmax 0.25, rowsum 0.030, Y 0.027, dot 0.27, dQ 0.048, dE 0.071, dK 0.061,
dV 0.073."""
import ctypes as C

import numpy as np
import pytest

from tests import attn_ref as ar
from tests import edge_softmax_ref as er
from tests.helpers import synth
from tests.test_gpu_gat_fused import dev, env, held, host, per_feature  # noqa: F401 (env: the module fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64), (8, 8), (4, 6), (2, 128)]   # (4, 6): scalar loads
EDGE = [False, True]


@pytest.fixture(scope="module")
def pat(env):
    rp, ci, _ = er.pattern_a()
    nnz = len(ci)
    eidx = np.random.default_rng(5).permutation(nnz).astype(np.int32)
    return dict(rp=rp, ci=ci, rows=er.row_of_entries(rp), eidx=eidx, n=len(rp) - 1, nc=er.N_COLS_A, nnz=nnz, d=np.diff(rp),
                rp_d=dev(env, rp), ci_d=dev(env, ci), eidx_d=dev(env, eidx))


def operands(H, D, n_q, n_k, n_e, edge, values=None):
    """float32 Q, G [n_q, F], K, V [n_k, F], E [n_e, F] or None; values: draw from these instead of uniform(-1, 1)"""
    rng = np.random.default_rng(1000 * H + D)
    f = (lambda *s: rng.uniform(-1, 1, s).astype(np.float32)) if values is None else (lambda *s: rng.choice(values, s).astype(np.float32))
    return dict(Q=f(n_q, H * D), G=f(n_q, H * D), K=f(n_k, H * D), V=f(n_k, H * D), E=f(n_e, H * D) if edge else None)


def padded(t, bufs):
    """t on a pitch of F + 3 at a base 4 bytes off alignment, between NaN pads (kept in bufs) -- the scalar load and store path"""
    rows, F = t.shape
    buf = t.new_full((rows * (F + 3) + 1,), float("nan"))
    view = buf[1:].view(rows, F + 3)[:, :F]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    bufs.append(buf)
    return view


def pads_kept(bufs, F):
    return all(bool(b[0].isnan() and b[1:].view(-1, F + 3)[:, F:].isnan().all()) for b in bufs)


def forward_on(env, pat, o, H, scale=None, wrap=lambda t: t, out=None):
    dv = {k: None if v is None else wrap(dev(env, v)) for k, v in o.items()}
    Y, m, z = env["ops"].attn_aggregate(pat["rp_d"], pat["ci_d"], dv["Q"], dv["K"], dv["V"], H, E=dv["E"],
                                        eidx=None if o["E"] is None else pat["eidx_d"], scale=scale, out=out)
    return host(Y), host(m), host(z)


@pytest.mark.parametrize("edge", EDGE, ids=["plain", "edge"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_forward_exact(env, pat, H, D, edge):
    """Q = 0: every score is +0, every x is 1, z is the row length and Y = float32(sum) / float32(d) bit for bit in any order -- a dropped,
    doubled or mis-segmented entry, or a rescale factor that is not exactly 1, fails it."""
    o = operands(H, D, pat["n"], pat["nc"], pat["nnz"], edge, values=[-1.0, 0.0, 1.0])
    o["Q"][:] = 0
    Y, m, z = forward_on(env, pat, o, H)
    d, some = pat["d"], pat["d"] > 0
    vp = o["V"][pat["ci"]].astype(np.float64) + (o["E"][pat["eidx"]] if edge else 0)
    total = np.zeros((pat["n"], H * D))
    np.add.at(total, pat["rows"], vp)
    assert np.array_equal(z, np.repeat(d[:, None], H, 1).astype(np.float32)) and not np.signbit(z).any()
    assert np.all(m[some] == 0) and np.all(np.isneginf(m[~some]))
    assert np.array_equal(Y[some], total[some].astype(np.float32) / d[some, None].astype(np.float32))
    assert np.all(Y[~some] == 0) and not np.signbit(Y[~some]).any()


CASES = [(h, d, e, False, 1.0) for h, d in SHAPES for e in EDGE] + [(8, 8, True, True, 1.0), (8, 8, True, False, 60.0)]


@pytest.mark.parametrize("H,D,edge,offset,qscale", CASES, ids=[f"{h}x{d}-{'edge' if e else 'plain'}{'-offset' * o}{'-q60' * (q > 1)}" for h, d, e, o, q in CASES])
def test_forward(env, pat, H, D, edge, offset, qscale):
    """General data; qscale = 60 makes scores whose expf overflows unless the maximum is subtracted.  offset: every matrix, Y included, on
    a pitch of F + 3 at a base 4 bytes off alignment, between NaN pads that must survive."""
    o = operands(H, D, pat["n"], pat["nc"], pat["nnz"], edge)
    o["Q"] *= np.float32(qscale)
    scale = D ** -0.5
    bufs = []
    wrap = (lambda t: padded(t, bufs)) if offset else (lambda t: t)
    Y, m, z = forward_on(env, pat, o, H, scale, wrap, wrap(dev(env, np.zeros((pat["n"], H * D), np.float32))) if offset else None)
    assert pads_kept(bufs, H * D)
    ref = ar.forward(pat["rows"], pat["ci"], pat["eidx"], pat["n"], o["Q"], o["K"], o["V"], o["E"], H, float(np.float32(scale)))
    d, some = pat["d"], pat["d"] > 0
    assert np.all(np.isfinite(Y)) and np.all(np.isneginf(m[~some])) and np.all(z[~some] == 0)
    held(m[some], ref["m"][some], ar.c_s(D), ref["S_m"][some], "rowmax")
    held(z, ref["z"], per_feature(ar.c_z(d, D), pat["n"]), ref["S_z"], "rowsum")
    held(Y, ref["Y"], per_feature(ar.c_Y(d, D), pat["n"]), ref["S_Y"], "Y")


@pytest.mark.parametrize("H,D,edge,offset", [c[:4] for c in CASES[:-1]],
                         ids=[f"{h}x{d}-{'edge' if e else 'plain'}{'-offset' * o}" for h, d, e, o, _ in CASES[:-1]])
def test_backward(env, pat, H, D, edge, offset):
    """offset: every [rows, F] matrix, the outputs included, on the pitch of test_forward's offset case; the pads must survive."""
    ops, torch = env["ops"], env["torch"]
    bufs = []
    wrap = (lambda t: padded(t, bufs)) if offset else (lambda t: t)
    given = lambda a: wrap(dev(env, a)) if offset else None   # noqa: E731  an output the caller hands in, on the pitch
    n, nc, nnz, d, F = pat["n"], pat["nc"], pat["nnz"], pat["d"], H * D
    scale = float(np.float32(D ** -0.5))
    eidx_d = pat["eidx_d"] if edge else None
    # row side: A is the forward pattern; Y, m, z are the float32 roundings of the reference forward (an empty row's z is never read)
    o = operands(H, D, n, nc, nnz + 5, edge)
    ent = (pat["rows"], pat["ci"], pat["eidx"])
    fw = ar.forward(*ent, n, o["Q"], o["K"], o["V"], o["E"], H, scale)
    Y, m, z = (fw[k].astype(np.float32) for k in ("Y", "m", "z"))
    ref = ar.backward(*ent, n, nc, o["G"], o["Q"], o["K"], o["V"], o["E"], H, scale, m, z, Y=Y)
    dv = {k: None if v is None else wrap(dev(env, v)) for k, v in o.items()}
    sentinel = wrap(torch.full((nnz + 5, F), 7.0, device=env["dev"])) if edge else None
    dQ, dot, dE = ops.attn_aggregate_bwd_rows(pat["rp_d"], pat["ci_d"], dv["G"], dv["Q"], dv["K"], dv["V"], wrap(dev(env, Y)), H, dev(env, m), dev(env, z),
                                              E=dv["E"], eidx=eidx_d, scale=scale, dq_out=given(np.zeros((n, F), np.float32)), de_out=sentinel)
    held(host(dot), ref["dot"], ar.dot_chain(D), ref["S_dot"], "dot")   # the dot's chain alone
    held(host(dQ), ref["dQ"], per_feature(ar.c_dQ(d, D), n), ref["S_dQ"], "dQ")
    assert np.all(host(dQ)[d == 0] == 0)
    if edge:
        held(host(dE)[pat["eidx"]], ref["dE"], ar.c_dE(D), ref["S_dE"], "dE")
        assert np.all(host(dE)[nnz:] == 7.0)   # rows that no entry names keep the sentinel

    # column side: A is the TRANSPOSED pattern, so its hub rows are this call's; the rows i of A^T own Q, G, m, z and dot
    o = operands(H, D, nc, n, nnz, edge)
    ent = (pat["ci"], pat["rows"], pat["eidx"])
    fw = ar.forward(*ent, nc, o["Q"], o["K"], o["V"], o["E"], H, scale)
    m, z = fw["m"].astype(np.float32), fw["z"].astype(np.float32)
    dot = np.random.default_rng(D).uniform(-1, 1, (nc, H)).astype(np.float32)
    ref = ar.backward(*ent, nc, n, o["G"], o["Q"], o["K"], o["V"], o["E"], H, scale, m, z, dot=dot)
    dv = {k: None if v is None else wrap(dev(env, v)) for k, v in o.items()}
    old = np.random.default_rng(H).uniform(-1, 1, (2, n, F)).astype(np.float32)
    for beta in (0.0, 1.0):
        dK, dV = ops.attn_aggregate_bwd_cols(pat["rp_d"], pat["ci_d"], dv["G"], dv["Q"], dv["K"], dv["V"], H, dev(env, m), dev(env, z), dev(env, dot),
                                             E=dv["E"], eidx_t=eidx_d, scale=scale, dk_out=wrap(dev(env, old[0])), dv_out=wrap(dev(env, old[1])), beta=beta)
        held(host(dK), ref["dK"] + beta * old[0], per_feature(ar.c_dK(d, D), n), ref["S_dK"] + beta * np.abs(old[0]), f"dK beta={beta}")
        held(host(dV), ref["dV"] + beta * old[1], per_feature(ar.c_dV(d, D), n), ref["S_dV"] + beta * np.abs(old[1]), f"dV beta={beta}")
    assert pads_kept(bufs, F)


def test_two_runs_give_the_same_bits(env, pat):
    ops, torch, (H, D) = env["ops"], env["torch"], (8, 8)
    o = {k: dev(env, v) for k, v in operands(H, D, pat["n"], pat["nc"], pat["nnz"], True).items()}
    t = {k: dev(env, v) for k, v in operands(H, D, pat["nc"], pat["n"], pat["nnz"], True).items()}
    stat = torch.ones((pat["nc"], H), device=env["dev"])
    runs = []
    for _ in range(2):
        Y, m, z = ops.attn_aggregate(pat["rp_d"], pat["ci_d"], o["Q"], o["K"], o["V"], H, E=o["E"], eidx=pat["eidx_d"])
        dQ, dot, dE = ops.attn_aggregate_bwd_rows(pat["rp_d"], pat["ci_d"], o["G"], o["Q"], o["K"], o["V"], Y, H, m, z, E=o["E"], eidx=pat["eidx_d"])
        dK, dV = ops.attn_aggregate_bwd_cols(pat["rp_d"], pat["ci_d"], t["G"], t["Q"], t["K"], t["V"], H, stat * 5, stat, stat, E=t["E"],
                                             eidx_t=pat["eidx_d"])
        runs.append((Y, m, z, dQ, dot, dE, dK, dV))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- TransformerStack ------------------------------------------------------------------------------------------------------------
N, NE, DIMS, HEADS = 1 << 10, 8000, [32, 32, 8], [4, 1]


def model64(torch, rowptr, colidx, entry_edge, attr, X, params, rows, target):
    """The layers of TransformerStack in float64 autograd and the loss kernel's form of the cross entropy."""
    rows_e, cols_e = torch.from_numpy(er.row_of_entries(rowptr)), torch.from_numpy(colidx.astype(np.int64))
    h, L = torch.from_numpy(X.astype(np.float64)), len(HEADS)
    for l, Hh in enumerate(HEADS):
        F = DIMS[l + 1]
        Q, K, V, S = (h @ params["W"][l].T).split(F, dim=1)
        El = 0.0 if attr is None else (torch.from_numpy(attr.astype(np.float64)) @ params["W_e"][l].T)[torch.from_numpy(entry_edge.astype(np.int64))]
        kp, vp = K[cols_e] + El, V[cols_e] + El
        s = (Q[rows_e] * kp).reshape(-1, Hh, F // Hh).sum(2) * (F // Hh) ** -0.5
        m = torch.full((N, Hh), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, Hh), s.detach(), "amax")
        x = torch.exp(s - m[rows_e])
        alpha = x / torch.zeros((N, Hh), dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        Z = torch.zeros_like(Q).index_add(0, rows_e, alpha.repeat_interleave(F // Hh, 1) * vp) + S + params["b"][l]
        h = torch.relu(Z) if l + 1 < L else Z
    z = h[torch.from_numpy(rows.astype(np.int64))]
    picked = z[torch.arange(len(rows)), torch.from_numpy(target.astype(np.int64))[rows]]
    return h, (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(rows)


def close(got, r):
    return np.abs(got - r).max() <= 2e-5 * max(np.abs(r).max(), 1e-3)


@pytest.mark.parametrize("edge_dim", [None, 4], ids=["plain", "edge_dim_4"])
def test_stack_step_vs_float64(env, edge_dim):
    """One training step (lr = 0) against float64 autograd at the bars of tests/test_gpu_gat.py::test_one_step_vs_float64: 1e-5 *
    max(1, |ref|) on the loss, 2e-5 * max(|ref|_max, 1e-3) on the logits and every gradient, each non-zero in the reference."""
    ops, torch = env["ops"], env["torch"]
    src, dst = synth.rmat_edges(91, N, NE)
    s, d = dev(env, src), dev(env, dst)
    g = ops.CsrGraph.from_coo(s, d, N)
    attr = None
    if edge_dim:
        attr = synth.uniform_pm1(97, (NE, edge_dim))
        g.set_edge_attr(s, d, dev(env, attr))
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target, rows = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32), np.arange(0, N, 3, dtype=np.int32)
    net = ops.TransformerStack(g, DIMS, heads=HEADS, edge_dim=edge_dim, seed=950)
    assert edge_dim or getattr(g, "_map_t", None) is None   # no transpose map without edge features
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    names = ("W", "W_e", "b") if edge_dim else ("W", "b")
    params = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in names}
    loss = net.train_step(dev(env, X), dev(env, target), dev(env, rows), lr=0.0)
    logits = host(net.forward(dev(env, X)))
    logits_ref, ref = model64(torch, host(g.rowptr), host(g.colidx), host(g.entry_edge) if edge_dim else None, attr, X, params, rows, target)
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for k in names:
        for l in range(len(net.W)):
            r = params[k][l].grad.numpy()
            assert np.abs(r).max() > 0 and close(host(getattr(net, "d" + k)[l]), r), f"d{k}{l}"
    assert close(logits, logits_ref.detach().numpy())


def test_relabelled_graph(env):
    """Without edge features the stack takes a relabelled graph (rows in original-id order, which the transpose map refuses): one step
    gives, through g.nid, the logits and gradients of the same stack on the plain graph, at the bars of test_stack_step_vs_float64."""
    ops = env["ops"]
    src, dst = synth.rmat_edges(91, N, NE)
    X, target = dev(env, synth.uniform_pm1(93, (N, DIMS[0]))), dev(env, ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32))
    rows = dev(env, np.arange(0, N, 3, dtype=np.int32))
    out = []
    for relabel in (None, "scramble"):
        g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N, relabel=relabel)
        net = ops.TransformerStack(g, DIMS, heads=HEADS, seed=950)
        r = rows if relabel is None else g.nid[rows.long()].contiguous()
        loss = net.train_step(g.to_new_order(X), g.to_new_order(target), r, lr=0.0)
        out.append([host(loss), host(g.to_vertex_order(net.forward(g.to_new_order(X))))] + [host(t) for t in net.grads()])
    assert out[1][0] == pytest.approx(out[0][0], rel=1e-5)
    for a, b in zip(out[0][1:], out[1][1:]):
        assert close(b, a)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
FWD, ROWS, COLS = "gnnx_attn_csr_f32", "gnnx_attn_bwd_rows_csr_f32", "gnnx_attn_bwd_cols_csr_f32"
REFUSALS = [(FWD, dict(n_rows=-1), -1), (FWD, dict(nnz=2 ** 31), -1), (FWD, dict(H=0), -1), (ROWS, dict(D=0), -1), (FWD, dict(ldk=15), -1),
            (ROWS, dict(ldo=15), -1), (COLS, dict(lde=15), -1), (COLS, dict(beta=2.0), -1), (FWD, dict(null="E"), -1), (ROWS, dict(null="eidx", ne=7), -1),
            (FWD, dict(null="Q"), -1), (ROWS, dict(null="rowmax"), -1), (COLS, dict(null="O2"), -1), (FWD, dict(null="rowptr"), -1),
            (FWD, dict(D=257), -7), (ROWS, dict(D=257), -7), (COLS, dict(H=65536, D=256), -7), (FWD, dict(ws_bytes=64), -4), (ROWS, dict(null="ws"), -4),
            (COLS, dict(ws_bytes=64), -4)]


@pytest.mark.parametrize("call,change,status", REFUSALS, ids=[f"{c[10:-8] or 'fwd'}-" + "_".join(f"{a}_{b}" for a, b in k.items()) for c, k, _ in REFUSALS])
def test_refusals_write_nothing(env, pat, call, change, status):
    """Every status the header lists (valid arguments of (H, D) = (2, 8) on pattern A with one change; O, O2 stand for the call's [rows, F]
    outputs, ldo for their leading dimension; null="E" leaves eidx without edge rows, null="eidx" with ne=7 leaves too few edge rows):
    the call returns it and every sentinel-filled array, outputs included, keeps its bits."""
    torch, L = env["torch"], env["capi"].lib()
    v = dict(n_rows=pat["n"], nnz=pat["nnz"], H=2, D=8, ld=16, ldk=16, lde=16, ldo=16, ne=pat["nnz"], beta=0.0, null=None, ws_bytes=1 << 24)
    v.update(change)
    if v["H"] > 2:   # the passes limit: consistent leading dimensions, so that only the limit refuses
        v.update({k: v["H"] * v["D"] for k in ("ld", "ldk", "lde", "ldo")})
    t = {k: torch.full((pat["nc"], 16), 7.0, device=env["dev"]) for k in ("G", "Q", "K", "V", "E", "Y", "rowmax", "rowsum", "dot", "O", "O2", "dE")}
    t["ws"] = torch.full((1 << 22,), 7.0, device=env["dev"])
    ptrs = dict(t, rowptr=pat["rp_d"], eidx=pat["eidx_d"])
    P = lambda k: None if v["null"] == k else C.c_void_p(ptrs[k].data_ptr())  # noqa: E731
    head = [v["n_rows"], pat["nc"], v["nnz"], P("rowptr"), C.c_void_p(pat["ci_d"].data_ptr()), P("eidx"), v["ne"], v["H"], v["D"], 0.25]
    mats = [P("Q"), v["ld"], P("K"), v["ldk"], P("V"), v["ld"], P("E"), v["lde"]]
    tail = [P("ws"), v["ws_bytes"], None]
    if call == FWD:
        rc = getattr(L, call)(*head, *mats, P("O"), v["ldo"], P("rowmax"), P("rowsum"), *tail)
    elif call == ROWS:
        rc = getattr(L, call)(*head, P("G"), v["ld"], *mats, P("Y"), v["ld"], P("rowmax"), P("rowsum"), P("O"), v["ldo"], P("dot"), P("dE"), v["ldo"], *tail)
    else:
        rc = getattr(L, call)(*head, P("G"), v["ld"], *mats, P("rowmax"), P("rowsum"), P("dot"), v["beta"], P("O"), v["ldo"], P("O2"), v["ldo"], *tail)
    torch.cuda.synchronize()
    assert rc == status
    assert all(bool((a == 7.0).all()) for a in t.values())
