"""GPU tests of the optimiser kernels (gnn.cpp_amd/csrc/gnnx_optim.hip) and of ops.Adam / ops.Momentum (run with -m gpu on an MI355X)
against tests/optim_ref.py: every update bit for bit, the gradient norm by equality on data whose sum is exact in any order and
bit for bit against the documented order on general data, NaN-filled pads around every view.

Which path a table reaches (a chunk is 1024 elements, one workgroup):
  TABLE_ONE   (1025,)                     two chunks of one tensor: a full float4 chunk and a chunk that is one scalar tail element
  TABLE_NINE  1, 3, 4, 5, 0, 1023, 1024, 1025, 2049    tail only (1, 3), one float4 lane (4), a lane and a tail (5), no chunk (0), 255
              lanes and a 3-element tail (1023), three chunks (2049); the state offsets are rounded up to 4, so the arena has gaps
  TABLE_MANY  300 tensors of 1 .. 7 elements: 300 chunks -- the binary search over the prefix array, 9 levels
  shifted     TABLE_NINE with the parameter views, the gradient views or both one float off the 16-byte grid: every chunk on scalar lanes
Each update runs three consecutive steps (the momentum buffer's first step and two later ones; Adam's t = 1, 2, 3), with and without
a scale read from the device."""
import ctypes as C
import functools
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import elementwise_ref as E
from tests import norm_ref as R
from tests import optim_ref as O
from tests.helpers import ROOT, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN_WORD = 0x7FC00000
LR, B1, B2, EPS, WD = 0.01, 0.9, 0.999, 1e-8, 0.05
SCALE = 0.37
TABLES = {"one": (O.TABLE_ONE, ""), "nine": (O.TABLE_NINE, ""), "many": (O.TABLE_MANY, ""), "nine_p_off": (O.TABLE_NINE, "p"),
          "nine_g_off": (O.TABLE_NINE, "g"), "nine_pg_off": (O.TABLE_NINE, "pg")}
UPDATES = {"adam_coupled": dict(kind="adam", wd=WD, decoupled=False), "adamw": dict(kind="adam", wd=WD, decoupled=True),
           "adam_wd0": dict(kind="adam", wd=0.0, decoupled=False),
           "momentum": dict(kind="momentum", wd=WD, momentum=0.9, dampening=0.0, nesterov=False),
           "momentum_dampened": dict(kind="momentum", wd=0.0, momentum=0.9, dampening=0.25, nesterov=False),
           "nesterov": dict(kind="momentum", wd=WD, momentum=0.8, dampening=0.0, nesterov=True)}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def host(t):
    return t.detach().cpu().numpy()


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def words(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ a table on the device
class Slab:
    """Tensors of `sizes` as views of ONE NaN-filled device buffer: each view starts on the 16-byte grid (or one float behind it with
    `off`), with at least four NaN words between neighbours.  set() writes the views, expected() is the whole buffer as it must look."""

    def __init__(self, env, sizes, off=False):
        self.env, self.sizes = env, list(sizes)
        self.pos, cur = [], 4
        for n in sizes:
            self.pos.append(cur + (1 if off else 0))
            cur = (cur + n + 1 + 3) // 4 * 4 + 4
        self.host = np.full(cur + 4, np.nan, dtype=np.float32)
        assert (words(self.host) == NAN_WORD).all()
        self.buf = dev(env, self.host)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[p:p + n] for p, n in zip(self.pos, sizes)]
        for v, n in zip(self.views, sizes):
            assert n == 0 or (v.data_ptr() % 16 != 0) == off

    def set(self, arrays):
        for p, a in zip(self.pos, arrays):
            self.host[p:p + len(a)] = a
        self.buf.copy_(dev(self.env, self.host))

    def check(self, arrays, what):
        """The views hold `arrays` and every other word is still the NaN it was, by bit pattern."""
        want = np.full_like(self.host, np.nan)
        for p, a in zip(self.pos, arrays):
            want[p:p + len(a)] = a
        got = host(self.buf)
        bad = np.nonzero(~((words(got) == words(want)) | (np.isnan(got) & np.isnan(want))))[0]
        assert not len(bad), f"{what}: {len(bad)} words differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}"
        pads = np.ones(len(want), dtype=bool)
        for p, a in zip(self.pos, arrays):
            pads[p:p + len(a)] = False
        assert (words(got)[pads] == NAN_WORD).all(), f"{what}: a pad word changed"


class Table:
    """gnnx_optim_table_build over two Slabs, and guarded zeroed state arenas."""

    def __init__(self, env, sizes, off="", n_state=2):
        self.env, self.sizes = env, list(sizes)
        torch, capi = env["torch"], env["capi"]
        self.p, self.g = Slab(env, sizes, "p" in off), Slab(env, sizes, "g" in off)
        n = len(sizes)
        nbytes, chunks, elems = C.c_size_t(0), C.c_int64(0), C.c_int64(0)
        capi.call("gnnx_optim_table_bytes", n, C.byref(nbytes))
        self.table = torch.empty(nbytes.value, dtype=torch.uint8, device=env["dev"])
        capi.call("gnnx_optim_table_build", n, (C.c_void_p * n)(*[v.data_ptr() for v in self.p.views]),
                  (C.c_void_p * n)(*[v.data_ptr() for v in self.g.views]), (C.c_int64 * n)(*sizes), self.table.data_ptr(), nbytes.value,
                  C.byref(chunks), C.byref(elems), None)
        self.n, self.chunks = n, chunks.value
        self.offsets, self.elems = O.state_offsets(sizes)
        assert elems.value == self.elems and self.chunks == sum(-(-s // 1024) for s in sizes)
        self.arena_host = [np.full(self.elems + 8, np.nan, dtype=np.float32) for _ in range(n_state)]
        for a in self.arena_host:
            a[4:4 + self.elems] = 0.0
        self.arena_buf = [dev(env, a) for a in self.arena_host]
        self.arena = [b[4:4 + self.elems] for b in self.arena_buf]      # 16-byte aligned: every tensor's state is
        torch.cuda.synchronize()

    def check_state(self, k, arrays, what):
        """Arena k holds `arrays` at the tensors' offsets, +0 in the rounding gaps, NaN in the guards."""
        want = self.arena_host[k].copy()
        for o, a in zip(self.offsets, arrays):
            want[4 + o:4 + o + len(a)] = a
        got = host(self.arena_buf[k])
        bad = np.nonzero(~((words(got) == words(want)) | (np.isnan(got) & np.isnan(want))))[0]
        assert not len(bad), f"{what}: {len(bad)} words differ, first at {bad[0] - 4}: got {got[bad[0]]!r}, want {want[bad[0]]!r}"

    def adam(self, t, lr=LR, wd=0.0, decoupled=False, scale=None):
        capi = self.env["capi"]
        c1, c2 = C.c_float(0), C.c_float(0)
        capi.call("gnnx_adam_bias_corrections", B1, B2, t, C.byref(c1), C.byref(c2))
        capi.call("gnnx_adam_step_f32", self.table.data_ptr(), self.n, self.chunks, self.arena[0].data_ptr(), self.arena[1].data_ptr(), lr, B1, B2,
                  EPS, c1.value, c2.value, wd, int(decoupled), None if scale is None else scale.data_ptr(), None)

    def momentum(self, first, lr=LR, momentum=0.9, dampening=0.0, nesterov=False, wd=0.0, scale=None):
        self.env["capi"].call("gnnx_momentum_step_f32", self.table.data_ptr(), self.n, self.chunks, self.arena[0].data_ptr(), lr, momentum, dampening,
                              int(nesterov), int(first), wd, None if scale is None else scale.data_ptr(), None)

    def sqnorm(self, max_norm, ws=None, nbytes=None):
        torch, L = self.env["torch"], self.env["capi"].lib()
        out = torch.full((2,), -1.0, dtype=torch.float32, device=self.env["dev"])
        ws = torch.empty(1024, dtype=torch.uint8, device=self.env["dev"]) if ws is None else ws
        st = L.gnnx_grad_sqnorm_f32(self.table.data_ptr(), self.n, max_norm, out.data_ptr(), out.data_ptr() + 4, ws.data_ptr(),
                                    1024 if nbytes is None else nbytes, None)
        return st, host(out)


def draw(sizes, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng([seed, len(sizes)])
    return [rng.uniform(lo, hi, n).astype(np.float32) for n in sizes]


# ------------------------------------------------------------------------------------------------ every update on every table
@pytest.mark.parametrize("update", list(UPDATES))
@pytest.mark.parametrize("table", list(TABLES))
def test_three_steps_equal_the_restatement(env, table, update):
    """p and m, v (or buf) after each of three steps, with and without a scale, equal optim_ref by bit pattern; the pads around every
    parameter and gradient view and the gaps and guards of the arenas keep their bits."""
    sizes, off = TABLES[table]
    u = dict(UPDATES[update])
    kind = u.pop("kind")
    for with_scale in (False, True):
        tb = Table(env, sizes, off, n_state=2 if kind == "adam" else 1)
        scale = dev(env, np.array([SCALE], dtype=np.float32)) if with_scale else None
        s = F32(SCALE) if with_scale else None
        p = draw(sizes, 1)
        tb.p.set(p)
        m, v = [np.zeros(n, dtype=np.float32) for n in sizes], [np.zeros(n, dtype=np.float32) for n in sizes]
        for step in (1, 2, 3):
            g = draw(sizes, 10 + step)
            tb.g.set(g)
            what = f"{table} {update} scale={with_scale} step {step}"
            if kind == "adam":
                tb.adam(step, scale=scale, **u)
                for k in range(len(sizes)):
                    O.no_subnormals(*O.adam_intermediates(p[k], g[k], m[k], v[k], LR, B1, B2, EPS, step, scale=s, **u))
                    p[k], m[k], v[k] = O.adam_ref(p[k], g[k], m[k], v[k], LR, B1, B2, EPS, step, scale=s, **u)
                tb.check_state(1, v, what + ": v")
            else:
                tb.momentum(step == 1, scale=scale, **u)
                for k in range(len(sizes)):
                    p[k], m[k] = O.momentum_ref(p[k], g[k], m[k], LR, first=step == 1, scale=s, **u)
                    O.no_subnormals(p[k], m[k])
            tb.p.check(p, what + ": p")
            tb.check_state(0, m, what + (": m" if kind == "adam" else ": buf"))
            tb.g.check(g, what + ": the gradients")


# ------------------------------------------------------------------------------------------------ single edges
def test_momentum_zero_is_sgd_step_by_bits(env):
    """momentum = 0, dampening = 0, no scale: the bits of gnnx_sgd_step_f32 on the edge data of test_axpy_fill_sgd (an infinite p, g = -0,
    wd = 0 skipping the decay term) -- on the first step and on a later one over the +0 buffer -- and with a decay."""
    ops, n = env["ops"], 257
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    p, g = y.copy(), x.copy()
    p[:3], g[:3] = (np.inf, -np.inf, 0.0), (1.0, -0.0, -0.0)
    for wd in (0.0, 5e-4):
        sgd = dev(env, p)
        ops.sgd_step(sgd, dev(env, g), 0.1, wd)
        R.assert_bits(host(sgd), E.sgd_ref(p, g, 0.1, wd), "sgd_step itself")
        for first in (True, False):
            tb = Table(env, (n,), n_state=1)
            tb.p.set([p])
            tb.g.set([g])
            tb.momentum(first, lr=0.1, momentum=0.0, wd=wd)
            tb.p.check([host(sgd)], f"momentum 0, wd={wd}, first={first}")
        if wd == 0.0:
            assert np.isinf(host(sgd)[:2]).all()


def test_zero_gradient_on_zero_state(env):
    """The padded columns of GcnStack.Wp: g = 0 on m = v = 0 leaves p with its bits (a -0 included) and m, v at +0."""
    sizes = (1025, 7)
    p = draw(sizes, 3)
    p[0][:4] = (0.0, -0.0, 1.5, -2.0)
    zeros = [np.zeros(n, dtype=np.float32) for n in sizes]
    for wd, dec in ((0.0, False), (0.0, True)):
        tb = Table(env, sizes)
        tb.p.set(p)
        tb.g.set(zeros)
        tb.adam(1, wd=wd, decoupled=dec)
        tb.p.check(p, "p")
        tb.check_state(0, zeros, "m")
        tb.check_state(1, zeros, "v")
    # with a decay a ZERO parameter still stays zero (wd * 0 = 0) and its moments at +0
    tb = Table(env, (8,))
    tb.p.set([np.zeros(8, dtype=np.float32)])
    tb.g.set([np.zeros(8, dtype=np.float32)])
    tb.adam(1, wd=WD)
    tb.p.check([np.zeros(8, dtype=np.float32)], "zero p under decay")
    tb.check_state(0, [np.zeros(8, dtype=np.float32)], "m under decay")


def test_non_finite_gradient_changes_its_own_element_only(env):
    """Without a scale a NaN and an Inf gradient element reach their own element of p, m, v (and buf) and no other bit."""
    sizes = (1025, 5)
    p, g = draw(sizes, 4), draw(sizes, 5)
    bad = [a.copy() for a in g]
    bad[0][3], bad[0][1024], bad[1][2] = np.nan, np.inf, -np.inf
    hit = [np.zeros(n, dtype=bool) for n in sizes]
    hit[0][[3, 1024]], hit[1][2] = True, True
    zeros = [np.zeros(n, dtype=np.float32) for n in sizes]
    clean = [O.adam_ref(p[k], g[k], zeros[k], zeros[k], LR, B1, B2, EPS, 1) for k in range(2)]
    tb = Table(env, sizes)
    tb.p.set(p)
    tb.g.set(bad)
    tb.adam(1)
    ref = [O.adam_ref(p[k], bad[k], zeros[k], zeros[k], LR, B1, B2, EPS, 1) for k in range(2)]
    for j, name in enumerate("pmv"):
        for k in range(2):
            assert np.array_equal(words(ref[k][j])[~hit[k]], words(clean[k][j])[~hit[k]]) and not np.isfinite(ref[k][j][hit[k]]).any(), name
    tb.p.check([r[0] for r in ref], "p")
    tb.check_state(0, [r[1] for r in ref], "m")
    tb.check_state(1, [r[2] for r in ref], "v")
    tm = Table(env, sizes, n_state=1)
    tm.p.set(p)
    tm.g.set(bad)
    tm.momentum(True)
    refm = [O.momentum_ref(p[k], bad[k], zeros[k], LR, 0.9, first=True) for k in range(2)]
    cleanm = [O.momentum_ref(p[k], g[k], zeros[k], LR, 0.9, first=True) for k in range(2)]
    for k in range(2):
        assert np.array_equal(words(refm[k][0])[~hit[k]], words(cleanm[k][0])[~hit[k]]) and not np.isfinite(refm[k][0][hit[k]]).any()
    tm.p.check([r[0] for r in refm], "momentum p")
    tm.check_state(0, [r[1] for r in refm], "buf")


# ------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("table", ["nine", "many", "nine_g_off"])
def test_sqnorm_is_exact_and_the_scale_is_the_restatement(env, table):
    """Gradients from {+-2^-1 .. +-2^-4}: d_sqnorm equals the float64 sum; d_gscale = min(1, max_norm / (sqrtf(sq) + 1e-6f)) by bits for a
    max_norm above the norm (1) and one below it."""
    sizes, off = TABLES[table]
    tb = Table(env, sizes, off, n_state=1)
    grads = O.norm_gradients(sizes)
    tb.g.set(grads)
    sq = O.sqnorm_exact_ref(grads)
    norm = float(np.sqrt(sq))
    for max_norm in (2.0 * norm, 0.25 * norm):
        st, out = tb.sqnorm(max_norm)
        assert st == 0 and out[0] == sq, (out[0], sq)
        want = O.gscale_ref(sq, max_norm)
        assert R.same_bits(out[1], want) and (want == 1.0) == (max_norm > norm), (out[1], want)
    tb.g.check(grads, "the gradients")


def test_sqnorm_on_general_data_has_the_documented_order_and_the_same_bits_twice(env):
    sizes = O.TABLE_NINE + (300_000,)                 # 304 chunks: workgroups 0 .. 47 take a second one
    tb = Table(env, sizes, n_state=1)
    grads = draw(sizes, 8)
    tb.g.set(grads)
    (st1, a), (st2, b) = tb.sqnorm(1.0), tb.sqnorm(1.0)
    assert st1 == 0 and st2 == 0 and np.array_equal(words(a), words(b))
    want = O.sqnorm_ordered_ref(grads)
    assert R.same_bits(a[0], want), (a[0], want)
    assert R.same_bits(a[1], O.gscale_ref(want, 1.0)) and a[1] < 1.0
    assert abs(float(want) - sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)) < 1e-5 * float(want)


def test_sqnorm_workspace_size(env):
    torch, capi = env["torch"], env["capi"]
    need = C.c_size_t(0)
    capi.call("gnnx_grad_sqnorm_workspace", C.byref(need))
    tb = Table(env, (5, 3), n_state=1)
    tb.g.set([np.full(5, 0.5, dtype=np.float32), np.full(3, -0.25, dtype=np.float32)])
    ws = torch.empty(need.value, dtype=torch.uint8, device=env["dev"])
    st, out = tb.sqnorm(10.0, ws=ws, nbytes=need.value)
    assert st == 0 and out[0] == 5 * 0.25 + 3 * 0.0625 and out[1] == 1.0
    st, out = tb.sqnorm(10.0, ws=ws, nbytes=need.value - 1)
    assert st == -4 and (out == -1.0).all()


# ------------------------------------------------------------------------------------------------ models
N, EDGES = 300, 2400
MAX_NORM = 0.005     # below the first step's gradient norm of each of these models (asserted), so the scale is a real factor


@functools.lru_cache(maxsize=1)
def node_task():
    src, dst = synth.uniform_edges(31, N, EDGES)
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)
    return src, dst, mask


def make_model(env, kind):
    """(model, step arguments before lr): two calls give two models with the same parameters, by seed."""
    ops = env["ops"]
    if kind == "clf":
        rng = np.random.default_rng(41)
        graphs = []
        for n in [int(v) for v in rng.integers(8, 40, size=12)]:
            a = np.concatenate([np.arange(1, n), rng.integers(0, n, n)]).astype(np.int32)
            b = np.concatenate([rng.integers(0, np.arange(1, n)), rng.integers(0, n, n)]).astype(np.int32)
            keep = a != b
            graphs.append((np.concatenate([a[keep], b[keep]]), np.concatenate([b[keep], a[keep]]), n))
        batch = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, d), n) for s, d, n in graphs])
        X = synth.uniform_pm1(43, (batch.n, 16))
        target = (np.arange(len(graphs)) % 3).astype(np.int32)
        clf = ops.GraphClassifier(ops.SageStack(batch, [16, 24, 8], aggr="mean", seed=7), batch, 3, pool="mean", seed=9)
        return clf, (dev(env, X), dev(env, target))
    src, dst, mask = node_task()
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    dims = [100, 100, 5] if kind == "gcn_padded" else [16, 24, 5]
    X = dev(env, synth.uniform_pm1(33, (N, dims[0])))
    target = dev(env, ((7 * np.arange(N) + 3) % dims[-1]).astype(np.int32))
    if kind in ("gcn", "gcn_padded"):
        net = ops.GcnStack(g, dims, seed=5, pad_streamed=(kind == "gcn_padded"))
        assert net.padded == (kind == "gcn_padded")
        return net, (net.pad_input(X), target, g.labelled(dev(env, mask)))
    net = ops.GatStack(g, dims, seed=5, heads=[2, 1]) if kind == "gat" else ops.SageStack(g, dims, aggr="max", seed=5)
    return net, (X, target, g.rows_of(dev(env, mask)))


def hand_gradients(ops, model, args):
    """The body of the model's train_step without its step: forward, loss, backward."""
    if isinstance(model, ops.GraphClassifier):
        X, target = args
        logits = model.forward(X)
        loss, d = ops.softmax_ce(logits, target, colsum_out=model.db_c, grad_out=model._tmp("dlogits", tuple(logits.shape)))
        model.backward(d, have_bias_grad=True)
        return loss
    X, target, selection = args
    rows, pruned = model._selected(selection)
    logits = model.forward(X, **pruned)
    loss, G = ops.softmax_ce_rows(logits, target, rows, colsum_out=model.db[-1], grad_out=model.masked_grad_buffer(selection))
    model.backward(G, input_grad=False, have_last_bias_grad=True, **pruned)
    return loss


def pads_are_zero(net):
    if not getattr(net, "padded", False):
        return True
    ok = True
    for l, w in enumerate(net.Wp):
        full = host(w).copy()
        full[:net.dims[l + 1], :net.dims[l]] = 0.0
        ok = ok and not words(full).any()         # +0 by bit pattern
    return ok


@pytest.mark.parametrize("kind", ["gcn", "gcn_padded", "gat", "sage_max", "clf"])
def test_three_adam_train_steps_equal_a_hand_loop(env, kind):
    """train_step with Adam, weight decay and clipping against the model's own forward / loss / backward on a second model with the same
    seed, the gradients read back, the norm in the documented order and optim_ref on every tensor: equal parameters by bits after
    each of three steps; the pads of Wp stay +0; the optimiser's state is the restatement's."""
    ops = env["ops"]
    a, args = make_model(env, kind)
    b, args_b = make_model(env, kind)
    opt = ops.Adam(max_grad_norm=MAX_NORM)
    assert a.set_optimizer(opt) is a
    sizes = [p.numel() for p in b.params()]
    m, v = [np.zeros(n, dtype=np.float32) for n in sizes], [np.zeros(n, dtype=np.float32) for n in sizes]
    for step in (1, 2, 3):
        loss_a = a.train_step(*args, LR, WD)
        loss_b = hand_gradients(ops, b, args_b)
        assert R.same_bits(host(loss_a), host(loss_b)), f"step {step}: the two models disagree before the update"
        grads = [host(t).ravel() for t in b.grads()]
        sq = O.sqnorm_ordered_ref(grads)
        s = O.gscale_ref(sq, MAX_NORM)
        assert R.same_bits(host(opt.sqnorm)[0], sq) and R.same_bits(host(opt.gscale)[0], s)
        if step == 1:
            assert s < 1.0, "the clip is not active: choose a smaller MAX_NORM"
        for k, (pt, g) in enumerate(zip(b.params(), grads)):
            new, m[k], v[k] = O.adam_ref(host(pt).ravel(), g, m[k], v[k], LR, B1, B2, EPS, step, wd=WD, scale=s)
            pt.copy_(dev(env, new.reshape(tuple(pt.shape))))
        for k, (pa, pb) in enumerate(zip(a.params(), b.params())):
            R.assert_bits(host(pa), host(pb), f"{kind} step {step} parameter {k}")
        assert pads_are_zero(a if kind != "clf" else a.net), f"{kind} step {step}: a pad of Wp is not +0"
    st = opt.state()
    assert st["t"] == 3 and opt.t == 3 and len(st["m"]) == len(sizes)
    for k in range(len(sizes)):
        R.assert_bits(host(st["m"][k]), m[k], f"m[{k}]")
        R.assert_bits(host(st["v"][k]), v[k], f"v[{k}]")


def test_momentum_train_steps_equal_a_hand_loop(env):
    ops = env["ops"]
    a, args = make_model(env, "gcn")
    b, args_b = make_model(env, "gcn")
    opt = ops.Momentum(momentum=0.9, dampening=0.1, nesterov=False)
    a.set_optimizer(opt)
    buf = [np.zeros(p.numel(), dtype=np.float32) for p in b.params()]
    for step in (1, 2, 3):
        a.train_step(*args, LR, WD)
        hand_gradients(ops, b, args_b)
        for k, (pt, gt) in enumerate(zip(b.params(), b.grads())):
            new, buf[k] = O.momentum_ref(host(pt).ravel(), host(gt).ravel(), buf[k], LR, 0.9, 0.1, first=step == 1, wd=WD)
            pt.copy_(dev(env, new.reshape(tuple(pt.shape))))
        for k, (pa, pb) in enumerate(zip(a.params(), b.params())):
            R.assert_bits(host(pa), host(pb), f"step {step} parameter {k}")
    for k, t in enumerate(opt.state()["buf"]):
        R.assert_bits(host(t), buf[k], f"buf[{k}]")


def test_no_optimizer_is_the_per_tensor_sgd_loop(env):
    """A model with no optimiser set (and one whose optimiser was set back to None) steps as before: sgd_step per tensor."""
    ops = env["ops"]
    a, args = make_model(env, "gcn_padded")
    b, args_b = make_model(env, "gcn_padded")
    c, args_c = make_model(env, "gcn_padded")
    c.set_optimizer(ops.Adam()).set_optimizer(None)
    assert a.optimizer is None and c.optimizer is None
    for step in (1, 2):
        a.train_step(*args, 0.05, 5e-4)
        c.train_step(*args_c, 0.05, 5e-4)
        hand_gradients(ops, b, args_b)
        for p, g in zip(b.params(), b.grads()):
            ref = E.sgd_ref(host(p), host(g), 0.05, 5e-4)
            ops.sgd_step(p, g, 0.05, 5e-4)
            R.assert_bits(host(p), ref, "sgd_step")
        for k, (pa, pb, pc) in enumerate(zip(a.params(), b.params(), c.params())):
            R.assert_bits(host(pa), host(pb), f"step {step} parameter {k}")
            R.assert_bits(host(pc), host(pb), f"step {step} parameter {k} after set_optimizer(None)")


def test_views_share_the_optimizer_and_its_state(env):
    """SageStack.on_graph and GraphClassifier.on_batch views made BEFORE set_optimizer step the same state: t counts the steps through
    either, and the parameters have the bits of stepping through the original alone."""
    ops = env["ops"]
    a, args = make_model(env, "sage_max")
    b, args_b = make_model(env, "sage_max")
    view = a.on_graph(a.g)                      # before
    oa, ob = ops.Adam(max_grad_norm=MAX_NORM), ops.Adam(max_grad_norm=MAX_NORM)
    a.set_optimizer(oa)
    b.set_optimizer(ob)
    later = a.on_graph(a.g)                     # after
    assert view.optimizer is oa and later.optimizer is oa
    for through in (a, view, later):
        through.train_step(*args, LR, WD)
        b.train_step(*args_b, LR, WD)
    assert oa.t == 3 and ob.t == 3
    for k, (pa, pb) in enumerate(zip(a.params(), b.params())):
        R.assert_bits(host(pa), host(pb), f"parameter {k}")
    for x, y in zip(oa.state()["v"], ob.state()["v"]):
        R.assert_bits(host(x), host(y), "v")

    clf, cargs = make_model(env, "clf")
    ref, rargs = make_model(env, "clf")
    cview = clf.on_batch(clf.batch)
    oc, orf = ops.Adam(), ops.Adam()
    clf.set_optimizer(oc)
    ref.set_optimizer(orf)
    assert cview.optimizer is oc and clf.net.optimizer is None        # the classifier owns the union; the stack's own slot is free
    for through in (clf, cview, clf.on_batch(clf.batch)):
        through.train_step(*cargs, LR, WD)
        ref.train_step(*rargs, LR, WD)
    assert oc.t == 3 and len(oc.state()["m"]) == len(clf.net.params()) + 2
    for k, (pa, pb) in enumerate(zip(clf.params(), ref.params())):
        R.assert_bits(host(pa), host(pb), f"classifier parameter {k}")


def test_a_moved_parameter_is_refused_by_name(env):
    ops, torch = env["ops"], env["torch"]
    a, args = make_model(env, "gcn")
    opt = ops.Adam()
    a.set_optimizer(opt)
    a.train_step(*args, LR)
    a.b[1] = torch.zeros_like(a.b[1])
    with pytest.raises(RuntimeError, match=r"parameter 3 has moved"):
        a.step(LR)
    assert opt.t == 1
    other, _ = make_model(env, "gat")
    with pytest.raises(RuntimeError, match=r"this step has \d+ tensors"):
        other.set_optimizer(opt).step(LR)


# ------------------------------------------------------------------------------------------------ the C++ mirror
CPP_SIZES = (5, 1030)


@functools.lru_cache(maxsize=1)
def cpp_driver_output():
    """tests/cpp/test_host_optim_gpu.cpp compiled into a temporary directory with the compile line of tests/cpp/Makefile, run once:
    {name: float32 array} of the lines `name n w0 w1 ...` (hex words) it prints."""
    pkg = os.path.join(ROOT, "gnn.cpp_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_host_optim_gpu")
        cc = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-ffp-contract=off", "-Wall", "-Wno-sign-compare",
                             "-I" + os.path.join(pkg, "host", "include"), "-I" + os.path.join(ROOT, "include"),
                             os.path.join(ROOT, "tests", "cpp", "test_host_optim_gpu.cpp"), "-o", exe, "-L" + pkg, "-l:libgnncpp_host.so",
                             "-l:libgnnx_hip.so", "-Wl,-rpath," + pkg], capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr
        run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for line in run.stdout.splitlines():
        name, n, *ws = line.split()
        assert len(ws) == int(n)
        out[name] = np.array([int(w, 16) for w in ws], dtype=np.uint32).view(np.float32)
    return out


def cpp_inputs():
    """The driver's data, restated: p[k][i] = ((i * 37 + 11 * k) % 64 - 32) / 64, gradient of step s: ((i * 29 + 7 * k + 13 * s) % 128 - 64) / 256."""
    p = [((np.arange(n) * 37 + 11 * k) % 64 - 32).astype(np.float32) / F32(64) for k, n in enumerate(CPP_SIZES)]
    g = [[((np.arange(n) * 29 + 7 * k + 13 * s) % 128 - 64).astype(np.float32) / F32(256) for k, n in enumerate(CPP_SIZES)] for s in (0, 1)]
    return p, g


def test_cpp_sgd_momentum_and_adam_equal_the_restatement_and_python(env):
    """nn::SGD (momentum 0.9, dampening 0.1, weight decay; then Nesterov) and nn::Adam for two steps on two small tensors with fixed
    gradients: the parameters equal optim_ref by bits, and the table calls driven from Python."""
    got = cpp_driver_output()
    p0, g = cpp_inputs()
    cases = {"sgd": dict(momentum=0.9, dampening=0.1, nesterov=False, wd=WD), "nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True, wd=0.0)}
    for name, u in cases.items():
        p, buf = [a.copy() for a in p0], [np.zeros(n, dtype=np.float32) for n in CPP_SIZES]
        tb = Table(env, CPP_SIZES, n_state=1)
        tb.p.set(p)
        for s in (0, 1):
            tb.g.set(g[s])
            tb.momentum(s == 0, **u)
            for k in range(2):
                p[k], buf[k] = O.momentum_ref(p[k], g[s][k], buf[k], LR, first=s == 0, **u)
        tb.p.check(p, f"python {name}")
        for k in range(2):
            R.assert_bits(got[f"{name}{k}"], p[k], f"nn::SGD {name} tensor {k}")
    p, m, v = [a.copy() for a in p0], [np.zeros(n, dtype=np.float32) for n in CPP_SIZES], [np.zeros(n, dtype=np.float32) for n in CPP_SIZES]
    tb = Table(env, CPP_SIZES)
    tb.p.set(p)
    for s in (0, 1):
        tb.g.set(g[s])
        tb.adam(s + 1)
        for k in range(2):
            p[k], m[k], v[k] = O.adam_ref(p[k], g[s][k], m[k], v[k], LR, B1, B2, EPS, s + 1)
    tb.p.check(p, "python adam")
    for k in range(2):
        R.assert_bits(got[f"adam{k}"], p[k], f"nn::Adam tensor {k}")
