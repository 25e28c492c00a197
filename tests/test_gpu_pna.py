"""Tests of the PNA aggregation (ops.spmm_pna / ops.spmm_pna_bwd / ops.PnaStack; include/gnnx.h "principal neighbourhood aggregation")
against a float64 NumPy restatement written here: a plain loop over rows with a first-wins arg.  The argument checks at the top need no
device; everything else is marked gpu (run with -m gpu on an MI355X).

The pattern is tests/test_gpu_reduce.py's pattern(): a square n = 9000 graph with rows of 2 S + 5, S and S + 1 entries, columns of 2 S + 5 and S
entries, empty rows and one-entry rows.  Exact legs use X from {-2, -1, -0, +0, 1, 2}: both sums are integers below 2^24, exact in
float32 in any order, so mean and std must be the float32 chain of the header from the exact sums, bit for bit (division and square
root are correctly rounded on the device).

Backward bound.  dX[c] = y0 + (a + x_c b): `a` is a chain of at most 3 adds per entry over min(d, S) entries plus one add per segment, b
one add per entry, then a product and two adds: every partial sum is at most sum|terms| (resp. sum|B|) in magnitude, so the error is at
most (3 d_t + 8) 2^-24 (sum|terms| + |x_c| sum|B|) with d_t = min(d, S) + segments, where with beta = 1 the matrix added to is one of the
terms (the last add rounds relative to |y0 + t|).  Worst observed err / bound on an MI355X: 0.18 (F = 132); the forward's mean 0.52, std 0.27."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from tests.helpers import pkg, synth  # noqa: F401
from tests.reduce_ref import SEG
from tests.test_gpu_reduce import bits, dev, host, pattern, placed, strided    # the pattern and the strided-view helpers of the reductions

gpu = pytest.mark.gpu
N, S, EPS = 9000, SEG, 1e-5
FWD_WIDTHS = (1, 3, 4, 13, 20, 30, 64, 68, 70, 132, 260)
BWD_WIDTHS = (1, 5, 13, 16, 64, 70, 132, 260)
FWD_LAYOUTS = ("x_off", "odd_ldx", "odd_ldy", "odd_lda", "arg_off")      # one failing vec4 condition each, at F = 64
BWD_LAYOUTS = ("dm_off", "odd_ldm", "odd_lda", "odd_ldx", "arg_off")
X_VALUES = np.array([-2, -1, -0.0, 0.0, 1, 2], dtype=np.float32)
f32 = np.float32


# ---- argument checks: before any device call ---------------------------------------------------------------------------------------
def test_arguments_are_checked_without_a_device():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module("gnncpp_amd.capi").lib()
    p = C.c_void_p(4096)          # never dereferenced: every call returns before its first device call

    def fwd(n=8, F=4, ldy=16, eps=EPS, ws=p):
        return L.gnnx_spmm_csr_pna_f32(n, 8, F, 16, p, p, p, F, eps, p, ldy, p, F, p, F, ws, 1 << 20, None)

    def bwd(n=8, F=4, ldm=16, ws=p):
        return L.gnnx_spmm_csr_pna_bwd_f32(n, 8, F, 16, p, p, p, p, F, p, F, p, F, p, F, p, ldm, p, F, 0.0, p, F, ws, 1 << 20, None)

    assert fwd(ldy=15) == -1 and fwd(eps=-1e-5) == -1 and fwd(n=-1) == -1 and fwd(ws=None) == -4
    assert bwd(ldm=15) == -1 and bwd(n=-1) == -1 and bwd(ws=None) == -4
    assert L.gnnx_pna_bwd_coeff_f32(8, 4, p, p, 15, p, 16, p, 4, p, 4, None) == -1
    assert L.gnnx_pna_bwd_coeff_f32(-1, 4, p, p, 16, p, 16, p, 4, p, 4, None) == -1


# ---- shared data -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def assert_same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@pytest.fixture(scope="module")
def graph(env):
    p = dict(pattern(), deg=np.diff(pattern()["rowptr"]), deg_t=np.diff(pattern()["rowptr_t"]))
    deg, deg_t = p["deg"], p["deg_t"]                    # every path at the smallest size, checked before any device call
    assert (deg == 0).sum() >= 20 and (deg == 1).sum() >= 20 and 4 <= np.median(deg[300:]) <= 8
    assert deg[0] == 2 * S + 5 and deg[1] == S and deg[2] == S + 1 and deg_t[3] == 2 * S + 5 and deg_t[4] == S
    for k in ("rowptr", "colidx", "rowptr_t", "colidx_t", "map_t"):
        p["d_" + k] = dev(env, p[k])
    return p


def row_sums(T, rowptr):
    """float64 [n, F]: the sum of T's rows b .. e - 1 per CSR row."""
    out = np.zeros((len(rowptr) - 1, T.shape[1]))
    has = np.diff(rowptr) > 0
    out[has] = 0.0 + np.add.reduceat(T.astype(np.float64), rowptr[:-1][has], axis=0)     # from +0, as every chain: a row of -0 sums to +0
    return out


@functools.lru_cache(maxsize=None)
def forward_ref(F, kind):
    """X and, in float64 / with X's own bits: s1, s2, sum|x|, min, max, argmin, argmax -- a plain loop over rows, the first winner kept."""
    p = pattern()
    X = np.random.default_rng(1000 + F).choice(X_VALUES, size=(N, F)) if kind == "small" else synth.uniform_pm1(31, (N, F))
    T = X[p["colidx"]]
    mn, mx = np.zeros((N, F), f32), np.zeros((N, F), f32)
    amin, amax = np.full((N, F), -1, np.int32), np.full((N, F), -1, np.int32)
    cols = np.arange(F)
    for i in np.nonzero(np.diff(p["rowptr"]))[0]:
        b, e = p["rowptr"][i], p["rowptr"][i + 1]
        lo, hi = np.argmin(T[b:e], axis=0), np.argmax(T[b:e], axis=0)     # the first occurrence; -0 and +0 tie
        mn[i], mx[i], amin[i], amax[i] = T[b:e][lo, cols], T[b:e][hi, cols], b + lo, b + hi
    T64 = T.astype(np.float64)
    return dict(X=X, s1=row_sums(T64, p["rowptr"]), s2=row_sums(T64 * T64, p["rowptr"]), sabs=row_sums(np.abs(T64), p["rowptr"]), mn=mn, mx=mx,
                amin=amin, amax=amax)


def run_forward(env, graph, F, kind, layout="aligned"):
    """(M, argmin, argmax) on the host after the checks every leg shares: min, max and both args exact, empty rows, untouched pad."""
    torch, r = env["torch"], forward_ref(F, kind)
    d_X = placed(env, r["X"], ld=F + 1 if layout == "odd_ldx" else None, off=1 if layout == "x_off" else 0)
    M, Mbuf = strided(env, N, 4 * F, torch.float32, float("nan"), ld=4 * F + 1 if layout == "odd_ldy" else None)
    amin, _ = strided(env, N, F, torch.int32, -7, ld=F + 1 if layout == "odd_lda" else None)
    amax, _ = strided(env, N, F, torch.int32, -7, off=1 if layout == "arg_off" else 0)
    env["ops"].spmm_pna(graph["d_rowptr"], graph["d_colidx"], d_X, eps=EPS, out=M, argmin_out=amin, argmax_out=amax)
    M, amin, amax = host(M), host(amin), host(amax)
    what = f"F={F} {kind} {layout}"
    assert np.array_equal(amin, r["amin"]) and np.array_equal(amax, r["amax"]), what
    assert_same_bits(M[:, F:2 * F], r["mn"], "min " + what)
    assert_same_bits(M[:, 2 * F:3 * F], r["mx"], "max " + what)
    empty = graph["deg"] == 0
    assert (bits(M[empty]) == 0).all() and (amin[empty] == -1).all() and (amax[empty] == -1).all(), what
    if layout == "odd_ldy":
        assert bool(torch.isnan(Mbuf.view(N, 4 * F + 1)[:, 4 * F]).all()), what
    return M


def chain32(s1, s2, deg):
    """The header's float32 chain from float32 sums: (mean, std), one rounding per operation; +0 for an empty row."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (f32(1) / deg.astype(f32))[:, None]
        mean, msq = s1 * r, s2 * r
        diff = msq - mean * mean
        std = np.sqrt(np.where(diff > 0, diff, f32(0)) + f32(EPS))
    have = (deg > 0)[:, None]
    assert mean.dtype == f32 and std.dtype == f32
    return np.where(have, mean, f32(0)), np.where(have, std, f32(0))


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,layout", [(F, "aligned") for F in FWD_WIDTHS] + [(64, lay) for lay in FWD_LAYOUTS])
def test_forward_exact(env, graph, F, layout):
    r = forward_ref(F, "small")
    assert r["sabs"].max() < 2 ** 24 and r["s2"].max() < 2 ** 24          # both sums are exact in float32 in any order
    M = run_forward(env, graph, F, "small", layout)
    mean, std = chain32(r["s1"].astype(f32), r["s2"].astype(f32), graph["deg"])
    assert_same_bits(M[:, :F], mean, f"mean F={F} {layout}")
    assert_same_bits(M[:, 3 * F:], std, f"std F={F} {layout}")


@gpu
@pytest.mark.parametrize("F", (4, 64))
def test_forward_general(env, graph, F):
    r, u = forward_ref(F, "uniform"), 2.0 ** -24
    M = run_forward(env, graph, F, "uniform").astype(np.float64)
    d = graph["deg"][:, None].astype(np.float64)
    inv = np.where(d > 0, 1 / np.maximum(d, 1), 0)
    mean, msq = r["s1"] * inv, r["s2"] * inv
    std = np.where(d > 0, np.sqrt(np.maximum(msq - mean * mean, 0) + EPS), 0)
    d_mean, d_msq = (d + 1) * u * r["sabs"] * inv, (d + 2) * u * r["s2"] * inv     # the squares carry one more rounding
    d_var = d_msq + 2 * np.abs(mean) * d_mean + 3 * u * msq
    d_std = d_var / np.maximum(std, 1e-300) + u * std
    e_mean, e_std = np.abs(M[:, :F] - mean), np.abs(M[:, 3 * F:] - std)
    print(f"F={F}: worst err/bound mean {np.max(e_mean / np.maximum(d_mean, 1e-300)):.3f}, std {np.max(e_std / np.maximum(d_std, 1e-300)):.3f}")
    assert (e_mean <= d_mean).all() and (e_std <= d_std).all()


# ---- backward --------------------------------------------------------------------------------------------------------------------------
def backward_terms(graph, A, B, dM, amin, amax, F):
    """float64 per transposed row: (sum of the terms of `a`, sum of their magnitudes, sum B, sum |B|)."""
    i, p = graph["colidx_t"], graph["map_t"][:, None]
    T = np.stack([A[i], np.where(amax[i] == p, dM[i, 2 * F:3 * F], 0), np.where(amin[i] == p, dM[i, F:2 * F], 0)]).astype(np.float64)
    rp = graph["rowptr_t"]
    return row_sums(T.sum(0), rp), row_sums(np.abs(T).sum(0), rp), row_sums(B[i], rp), row_sums(np.abs(B[i]), rp)


def run_backward(env, graph, F, layout="aligned"):
    torch, ops, capi = env["torch"], env["ops"], env["capi"]
    r = forward_ref(F, "uniform")
    d_X = dev(env, r["X"])
    M, amin, amax = ops.spmm_pna(graph["d_rowptr"], graph["d_colidx"], d_X, eps=EPS)
    dM, y0 = synth.uniform_pm1(50 + F, (N, 4 * F)), synth.uniform_pm1(51 + F, (N, F))
    d_dM = placed(env, dM, ld=4 * F + 1 if layout == "odd_ldm" else None, off=1 if layout == "dm_off" else 0)
    d_amin = placed(env, host(amin), ld=F + 1 if layout == "odd_lda" else None)
    d_amax = placed(env, host(amax), off=1 if layout == "arg_off" else 0)
    # the coefficient kernel against its float32 restatement, bit for bit
    A, B = torch.empty((N, F), device=env["dev"]), torch.empty((N, F), device=env["dev"])
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    capi.call("gnnx_pna_bwd_coeff_f32", N, F, ptr(graph["d_rowptr"]), ptr(M), 4 * F, ptr(d_dM), d_dM.stride(0), ptr(A), F, ptr(B), F, None)
    Mh, deg = host(M), graph["deg"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rr = (f32(1) / deg.astype(f32))[:, None]
        Br = (dM[:, 3 * F:] * rr) / Mh[:, 3 * F:]
        Ar = dM[:, :F] * rr - Br * Mh[:, :F]
    Ar, Br = np.where(deg[:, None] > 0, Ar, f32(0)), np.where(deg[:, None] > 0, Br, f32(0))
    assert Ar.dtype == f32
    assert_same_bits(host(A), Ar, f"A F={F} {layout}")
    assert_same_bits(host(B), Br, f"B F={F} {layout}")
    # dX against the float64 sum of the same float32 terms
    sa, sa_abs, sb, sb_abs = backward_terms(graph, Ar, Br, dM, host(amin), host(amax), F)
    x = r["X"].astype(np.float64)
    d_t = (np.minimum(graph["deg_t"], S) + -(-graph["deg_t"] // S))[:, None]
    worst = 0.0
    for beta in (0, 1):
        dX, buf = strided(env, N, F, torch.float32, float("nan"), ld=F + 1 if layout == "odd_ldx" else None)
        if beta:
            dX.copy_(dev(env, y0))
        ops.spmm_pna_bwd(graph["d_rowptr_t"], graph["d_colidx_t"], graph["d_map_t"], graph["d_rowptr"], d_X, M, d_amin, d_amax, d_dM, out=dX, beta=float(beta))
        ref = beta * y0 + (sa + x * sb)
        bound = (3 * d_t + 8) * 2.0 ** -24 * (sa_abs + beta * np.abs(y0) + np.abs(x) * sb_abs)
        err = np.abs(host(dX) - ref)                   # beta = 0 never reads the NaN it overwrites: a NaN fails the compare
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all(), f"F={F} {layout} beta={beta}: worst err/bound {worst:.3f}"
        if layout == "odd_ldx":
            assert bool(torch.isnan(buf.view(N, F + 1)[:, F]).all())
    return worst


@gpu
@pytest.mark.parametrize("F,layout", [(F, "aligned") for F in BWD_WIDTHS] + [(64, lay) for lay in BWD_LAYOUTS])
def test_backward_general(env, graph, F, layout):
    print(f"F={F} {layout}: worst err/bound {run_backward(env, graph, F, layout):.4f}")


@gpu
def test_backward_exact_on_integers(env, graph):
    """Integer coefficients handed to the backward kernel directly: dX equals the int64 evaluation, hub column and tie-routed args included."""
    ops, F = env["ops"], 68
    r, rng = forward_ref(F, "small"), np.random.default_rng(7)
    A, B = rng.integers(-2, 3, (N, F)).astype(f32), rng.integers(-1, 2, (N, F)).astype(f32)
    dM, y0 = rng.integers(-3, 4, (N, 4 * F)).astype(f32), rng.integers(-5, 6, (N, F)).astype(f32)
    sa, sa_abs, sb, sb_abs = backward_terms(graph, A, B, dM, r["amin"], r["amax"], F)
    assert (sa_abs + 2 * sb_abs + 5).max() < 2 ** 24
    ref = y0 + (sa + r["X"].astype(np.float64) * sb)
    dX = dev(env, y0)
    ops.spmm_pna_bwd(graph["d_rowptr_t"], graph["d_colidx_t"], graph["d_map_t"], graph["d_rowptr"], dev(env, r["X"]), dev(env, np.zeros((N, 4 * F), f32)),
                     dev(env, r["amin"]), dev(env, r["amax"]), dev(env, dM), out=dX, beta=1.0, _coeff=(dev(env, A), dev(env, B)))
    assert np.array_equal(host(dX).astype(np.int64), ref.astype(np.int64)) and np.abs(ref[3]).max() > 0


# ---- PnaStack --------------------------------------------------------------------------------------------------------------------------
NS, DIMS, LR = 600, [12, 16, 5], 0.05


@pytest.fixture(scope="module")
def task(env):
    rng = np.random.default_rng(11)
    row = np.repeat(np.arange(NS), np.arange(NS) % 41)                        # row v stores v % 41 neighbours
    # every row of two or more entries stores the columns 0 and 1, whose features are +1 and -1: its variance is at least 2 / d
    col = np.concatenate([np.concatenate([[0, 1][:v % 41], rng.choice(np.delete(np.arange(2, NS), max(v - 2, 0)), max(v % 41 - 2, 0), replace=False)])
                          if v % 41 != 1 else rng.choice(np.delete(np.arange(NS), v), 1) for v in range(NS)]).astype(np.int64)
    g = env["ops"].CsrGraph.from_coo(dev(env, row.astype(np.int32)), dev(env, col.astype(np.int32)), NS)
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    deg = np.diff(rowptr)
    assert deg.min() == 0 and deg.max() == 40 and (deg == 1).any()
    X = synth.uniform_pm1(93, (NS, DIMS[0]))
    X[0], X[1] = 1, -1
    return dict(g=g, rowptr=rowptr, colidx=colidx, deg=deg, X=X, target=((7 * np.arange(NS) + 3) % DIMS[-1]).astype(np.int32),
                rows=np.arange(0, NS, 3, dtype=np.int32))


def make_net(env, g, seed=950):
    net = env["ops"].PnaStack(g, DIMS, seed=seed)
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    return net


@gpu
def test_one_step_vs_float64(env, task):
    torch = env["torch"]
    net = make_net(env, task["g"])
    logd = np.log(task["deg"] + 1.0)
    assert abs(net.delta - logd.mean()) <= 1e-6 and net.scalers == ("identity", "amplification", "attenuation") and net.scale[0] is None
    assert np.allclose(host(net.scale[1]), logd / logd.mean(), rtol=1e-6) and (host(net.scale[2])[task["deg"] == 0] == 0).all()
    assert np.allclose(host(net.scale[2])[task["deg"] > 0], (logd.mean() / logd[task["deg"] > 0]), rtol=1e-6)
    t64 = lambda p: torch.tensor(host(p).astype(np.float64), requires_grad=True)  # noqa: E731
    W_s, W_n, b = [t64(p) for p in net.W_s], [[t64(p) for p in ws] for ws in net.W_n], [t64(p) for p in net.b]
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    # the float64 model: min and max through the device's saved args, sqrt(var + eps) unclamped
    rows_e = torch.from_numpy(np.repeat(np.arange(NS), task["deg"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    cols_pad = torch.cat([cols_e, torch.zeros(1, dtype=torch.int64)])
    deg = torch.from_numpy(task["deg"].astype(np.float64))[:, None]
    scale = [torch.ones(NS, 1, dtype=torch.float64)] + [torch.from_numpy(host(s).astype(np.float64))[:, None] for s in net.scale[1:]]
    h = torch.from_numpy(task["X"].astype(np.float64))
    for l in range(len(W_s)):
        picked = [torch.where(a >= 0, h.gather(0, cols_pad[a]), torch.zeros((), dtype=torch.float64))
                  for a in (torch.from_numpy(host(net._saved[l][k]).astype(np.int64)) for k in (2, 3))]
        zeros = torch.zeros((NS, h.shape[1]), dtype=torch.float64)
        mean = zeros.index_add(0, rows_e, h[cols_e]) / deg.clamp(min=1)
        var = zeros.index_add(0, rows_e, h[cols_e] ** 2) / deg.clamp(min=1) - mean ** 2
        assert l > 0 or bool((var.detach()[task["deg"] >= 2] > 1e-3).all())      # the input is generic: the clamp never acts on it
        assert bool((var.detach()[task["deg"] == 1] == 0).all())
        std = torch.where(deg > 0, torch.sqrt(var + EPS), torch.zeros((), dtype=torch.float64))
        M = torch.cat([mean, picked[0], picked[1], std], 1)
        Z = h @ W_s[l].T + sum(s * (M @ W.T) for s, W in zip(scale, W_n[l])) + b[l]
        h = torch.relu(Z) if l + 1 < len(W_s) else Z
    r = torch.from_numpy(task["rows"].astype(np.int64))
    z = h[r]
    picked = z[torch.arange(len(r)), torch.from_numpy(task["target"].astype(np.int64))[r]]
    ref = (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r)      # the loss kernel's form
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for got, want in zip(net.grads(), W_s + [w for ws in W_n for w in ws] + b):
        want = want.grad.numpy()
        err = np.abs(host(got) - want).max()
        print(f"{tuple(want.shape)}: err {err:.3e}, scale {np.abs(want).max():.3e}")
        assert np.abs(want).max() > 0 and err <= 2e-5 * max(np.abs(want).max(), 1e-3)


@gpu
def test_training_goes_down_repeats_and_rebinds(env, task):
    torch, ops = env["torch"], env["ops"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    runs = []
    for _ in range(2):
        net = make_net(env, task["g"])
        losses = [float(host(net.train_step(X, t, rows, lr=LR))[0]) for _ in range(30)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.params()]))
    assert runs[0][0] == runs[1][0] and all(torch.equal(p, q) for p, q in zip(runs[0][1], runs[1][1]))
    view = net.on_graph(task["g"].sample_neighbors(5, 3))
    assert all(p is q for p, q in zip(view.params(), net.params())) and view.delta == net.delta
    assert not torch.equal(view.scale[1], net.scale[1]) and not torch.equal(view.scale[2], net.scale[2])
    assert np.isfinite(float(host(view.train_step(X, t, rows, lr=LR))[0]))
    with pytest.raises(env["capi"].GnnxError, match="transposed"):
        ops.PnaStack(ops.CsrGraph(NS, task["g"].rowptr, task["g"].colidx), DIMS)


@gpu
def test_under_graph_classifier_on_a_batch(env):
    ops, rng = env["ops"], np.random.default_rng(5)
    sizes = [9, 14, 20, 11, 16, 25, 8, 13]
    graphs = [(dev(env, rng.integers(0, n, 4 * n).astype(np.int32)), dev(env, rng.integers(0, n, 4 * n).astype(np.int32)), n) for n in sizes]
    batch = ops.GraphBatch.from_graphs(graphs)
    clf = ops.GraphClassifier(ops.PnaStack(batch, DIMS, seed=3), batch, 3, pool="mean")
    X, target = dev(env, synth.uniform_pm1(77, (sum(sizes), DIMS[0]))), dev(env, (np.arange(len(sizes)) % 3).astype(np.int32))
    losses = [float(host(clf.train_step(X, target, lr=LR))[0]) for _ in range(20)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
