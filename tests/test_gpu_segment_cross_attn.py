"""GPU tests of the cross segment attention calls and of GraphClassifier's attention readout (run with -m gpu on an MI355X):
ops.segment_cross_attention / _bwd_rows / _bwd_cols against the float64 loops of tests/segment_cross_attn_ref.py, which also counts c.

KEYS: an empty key segment; 1, 31, 32 keys are one key tile, so three of the four wavefronts see no key of those queries; 33 is one tile
and one row, 129 four tiles and one row, 300 ten tiles.  n_seeds queries per segment.  The own tile is T queries, T a function of
(n_q, n_heads): 1 at the sizes of the first six cases (every workgroup owns one query and splits its keys); the last three repeat KEYS
until T = 8 (4158 queries) and T = 32 (16 632 queries of 33 per segment, every query segment crosses own tiles; 5467 one-query segments
at 3 heads, 32 segments share an own tile and the running tile number deals them over the wavefronts).  Each check prints the worst
fraction of its bar.  Observed on an MI355X (worst over all cases): rowmax 0.43, rowsum 0.027, Y 0.013, dot 0.48, dQ 0.021, dK 0.058,
dV 0.042; the readout against float64 autograd at most 0.016 (db_v)."""
import numpy as np
import pytest

from tests import segment_attn_ref as sr
from tests import segment_cross_attn_ref as cr
from tests.test_gpu_attn import operands, padded, pads_kept
from tests.test_gpu_gat_fused import dev, env, held, host, per_feature  # noqa: F401 (env: the module fixture)

pytestmark = pytest.mark.gpu

KEYS = [0, 1, 31, 32, 33, 129, 300]
# H, D, n_seeds, offset (pitch F + 3, base 4 bytes off: scalar loads), trailing rows that no segment holds, beta, spread scores, KEYS times
CASES = [(1, 4, 1, False, False, 0.0, False, 1), (3, 20, 3, False, False, 1.0, False, 1), (1, 32, 33, False, True, 0.0, False, 1),
         (1, 128, 3, False, False, 0.0, False, 1), (3, 4, 33, True, True, 1.0, False, 1), (1, 32, 1, False, False, 0.0, True, 1),
         (1, 32, 33, False, True, 0.0, False, 18), (1, 32, 33, False, False, 1.0, False, 72), (3, 4, 1, False, True, 0.0, False, 781)]
IDS = [f"{h}x{d}-s{s}{'-offset' * o}{'-trailing' * t}-beta{int(b)}{'-spread' * w}-x{n}" for h, d, s, o, t, b, w, n in CASES]


def problem(H, D, S, trailing, spread, times):
    """host operands, both segment arrays and the float64 reference of one case"""
    segptr = np.concatenate([[0], np.cumsum(KEYS * times)]).astype(np.int32)
    qsegptr = (S * np.arange(len(KEYS) * times + 1)).astype(np.int32)
    n_q, n_rows = int(qsegptr[-1]) + 3 * trailing, int(segptr[-1]) + 5 * trailing
    o = operands(H, D, n_q, n_rows, 0, False)
    scale = float(np.float32(D ** -0.5))
    if spread:   # every other key tile of a segment scores far below the rest: two of the four wavefronts hold maxima > 200 below m*
        within = np.concatenate([np.arange(k) for k in KEYS * times])
        o["Q"][:] = 60
        o["K"] = (np.abs(o["K"]) * np.where(within // 32 % 2, -1, 1)[:, None]).astype(np.float32)
        s = scale * o["Q"][-1].astype(np.float64) @ o["K"][segptr[-2]:segptr[-1]].astype(np.float64).T
        assert s.max() - s.min() > 200 and s[32:64].max() < s.max() - 200
    fw = cr.forward(segptr, qsegptr, o["Q"], o["K"], o["V"], H, scale)
    o["m"], o["z"], o["Y"] = (fw[k].astype(np.float32) for k in ("m", "z", "Y"))
    bw = cr.backward(segptr, qsegptr, o["G"], o["Q"], o["K"], o["V"], o["Y"], o["m"], o["z"], H, scale)
    return o, segptr, qsegptr, scale, {**fw, **bw}


def run(env, o, segptr, qsegptr, scale, ref, H, offset, beta, bufs):
    """the three device calls; the backward from the float32-rounded m, z, Y (and dot) of the reference"""
    ops, torch = env["ops"], env["torch"]
    wrap = (lambda t: padded(t, bufs)) if offset else (lambda t: t)
    nan = lambda a: wrap(torch.full(a.shape, float("nan"), device=env["dev"]))  # noqa: E731
    seg = (dev(env, segptr), dev(env, qsegptr))
    G, Q, K, V = (wrap(dev(env, o[k])) for k in "GQKV")
    old = np.random.default_rng(H).uniform(-1, 1, (2,) + o["K"].shape).astype(np.float32)
    Y, m, z = ops.segment_cross_attention(*seg, Q, K, V, H, scale=scale, out=nan(o["Q"]))
    stats = (dev(env, o["m"]), dev(env, o["z"]))
    dQ, dot = ops.segment_cross_attention_bwd_rows(*seg, G, Q, K, V, wrap(dev(env, o["Y"])), H, *stats, scale=scale, dq_out=nan(o["Q"]))
    dK, dV = ops.segment_cross_attention_bwd_cols(*seg, G, Q, K, V, H, *stats, dev(env, ref["dot"].astype(np.float32)), scale=scale, beta=beta,
                                                  dk_out=wrap(dev(env, old[0])) if beta else nan(o["K"]),
                                                  dv_out=wrap(dev(env, old[1])) if beta else nan(o["K"]))
    return {k: host(v) for k, v in dict(Y=Y, m=m, z=z, dQ=dQ, dot=dot, dK=dK, dV=dV).items()}, old


@pytest.mark.parametrize("H,D,S,offset,trailing,beta,spread,times", CASES, ids=IDS)
def test_against_float64(env, H, D, S, offset, trailing, beta, spread, times):
    o, segptr, qsegptr, scale, ref = problem(H, D, S, trailing, spread, times)
    n_q, n_rows, bufs = len(o["Q"]), len(o["K"]), []
    got, old = run(env, o, segptr, qsegptr, scale, ref, H, offset, beta, bufs)
    assert pads_kept(bufs, H * D)
    nk, ns = cr.lengths(segptr, qsegptr, n_q, n_rows)
    none = nk == 0   # the empty key segment's queries and the trailing ones: exactly Y = 0, m = -inf, z = 0, dQ = 0
    assert none.sum() == S * times + 3 * trailing and np.all(np.isneginf(got["m"][none])) and not got["z"][none].any()
    assert not got["Y"][none].any() and not got["dQ"][none].any()
    assert all(np.isfinite(got[k]).all() for k in ("Y", "z", "dQ", "dot", "dK", "dV")) and np.isfinite(got["m"][~none]).all()
    held(got["m"][~none], ref["m"][~none], sr.c_s(D), ref["S_m"][~none], "rowmax")
    held(got["z"], ref["z"], per_feature(cr.c_z(nk, D), n_q), ref["S_z"], "rowsum")
    held(got["Y"], ref["Y"], per_feature(cr.c_Y(nk, D), n_q), ref["S_Y"], "Y")
    held(got["dot"], ref["dot"], sr.c_dot(D), ref["S_dot"], "dot")
    held(got["dQ"], ref["dQ"], per_feature(cr.c_dQ(nk, D), n_q), ref["S_dQ"], "dQ")
    # A weight below 2^-126 is flushed or rounded as a subnormal: an ABSOLUTE error of up to 2^-126 that the relative bars do not hold,
    # and with one query a key's whole gradient is such a term (spread).  Per key it is at most 2^-126 * queries * (|dP| + |dot| <= 2 D)
    # * max|Q| (dK; dV's is smaller); S takes it divided by 2^-24, as c >= 1.
    tiny = 2.0 ** -102 * max(S, 1) * 2 * D * float(np.abs(o["Q"]).max())
    held(got["dK"], ref["dK"] + beta * old[0], per_feature(sr.c_dK(ns, D), n_rows), ref["S_dK"] + beta * np.abs(old[0]) + tiny, "dK")
    held(got["dV"], ref["dV"] + beta * old[1], per_feature(sr.c_dV(ns, D), n_rows), ref["S_dV"] + beta * np.abs(old[1]) + tiny, "dV")


def test_two_runs_give_the_same_bits(env):
    H, D, S, offset, trailing, beta, spread, times = CASES[6]
    o, segptr, qsegptr, scale, ref = problem(H, D, S, trailing, spread, times)
    a, b = (run(env, o, segptr, qsegptr, scale, ref, H, offset, beta, [])[0] for _ in range(2))
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def test_agrees_with_the_self_attention_call(env):
    """qsegptr == segptr: the cross calls and the dense calls compute the same function in two orders, each within its own bar of the
    float64 reference, so they differ by at most the sum of the two bars."""
    ops, H, D = env["ops"], 2, 16
    segptr = np.concatenate([[0], np.cumsum(KEYS)]).astype(np.int32)
    n = int(segptr[-1])
    o = operands(H, D, n, n, 0, False)
    scale = float(np.float32(D ** -0.5))
    ref = cr.forward(segptr, segptr, o["Q"], o["K"], o["V"], H, scale)
    m, z, Y = (ref[k].astype(np.float32) for k in ("m", "z", "Y"))
    ref.update(cr.backward(segptr, segptr, o["G"], o["Q"], o["K"], o["V"], Y, m, z, H, scale))
    sp, (G, Q, K, V) = dev(env, segptr), (dev(env, o[k]) for k in "GQKV")
    stats, dot = (dev(env, m), dev(env, z)), dev(env, ref["dot"].astype(np.float32))
    dense = (ops.segment_attention(sp, Q, K, V, H, scale=scale)[0], ops.segment_attention_bwd_rows(sp, G, Q, K, V, dev(env, Y), H, *stats, scale=scale)[0],
             *ops.segment_attention_bwd_cols(sp, G, Q, K, V, H, *stats, dot, scale=scale))
    cross = (ops.segment_cross_attention(sp, sp, Q, K, V, H, scale=scale)[0],
             ops.segment_cross_attention_bwd_rows(sp, sp, G, Q, K, V, dev(env, Y), H, *stats, scale=scale)[0],
             *ops.segment_cross_attention_bwd_cols(sp, sp, G, Q, K, V, H, *stats, dot, scale=scale))
    d = np.repeat(np.diff(segptr), np.diff(segptr))
    both = dict(Y=sr.c_Y(d, D) + cr.c_Y(d, D), dQ=sr.c_dQ(d, D) + cr.c_dQ(d, D), dK=2 * sr.c_dK(d, D), dV=2 * sr.c_dV(d, D))
    for k, a, b in zip(("Y", "dQ", "dK", "dV"), cross, dense):
        held(host(a), host(b).astype(np.float64), per_feature(both[k], n), ref["S_" + k], k)


def test_attention_readout(env):
    """GraphClassifier(pool=AttentionReadout(heads=2, n_seeds=2)) over a 2-layer GcnStack on 6 graphs against float64 autograd of the readout
    (the stack's output taken as given; its float64 gradient against what backward hands the stack).  Bar: 4 ulp of float32 per operation
    on the longest chain, relative to the largest reference entry.  A chain is at most the n = 124 vertices a parameter gradient sums over
    plus the 40 keys of the largest graph, the S F = 16 terms of a logit and the F = 8 terms of each of K, V and the scores: 204."""
    ops, torch = env["ops"], env["torch"]
    sizes, dims, C, (heads, S) = [5, 40, 17, 33, 8, 21], [6, 16, 8], 3, (2, 2)
    rng = np.random.default_rng(11)
    graphs = [(rng.integers(0, k, 3 * k).astype(np.int32), rng.integers(0, k, 3 * k).astype(np.int32), k) for k in sizes]
    g = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, t), k) for s, t, k in graphs])
    n, B, F = g.n, len(sizes), dims[-1]
    tol = 4 * 2.0 ** -24 * (n + max(sizes) + S * F + 3 * F)
    clf = ops.GraphClassifier(ops.GcnStack(g, dims, seed=3), g, C, pool=ops.AttentionReadout(heads, S), seed=1)
    names = ("W_c", "b_c", "P", "W_k", "b_k", "W_v", "b_v")
    mine, dmine = clf.params()[-7:], clf.grads()[-7:]
    for p in (mine[1], mine[4], mine[6]):   # the biases start at zero
        p.copy_(dev(env, rng.uniform(-0.3, 0.3, tuple(p.shape)).astype(np.float32)))
    X, dlogits = dev(env, rng.uniform(-1, 1, (n, dims[0])).astype(np.float32)), rng.uniform(-1, 1, (B, C)).astype(np.float32)
    logits = host(clf.forward(X))
    clf.backward(dev(env, dlogits))
    t = {k: torch.tensor(host(p).astype(np.float64), requires_grad=True) for k, p in zip(names, mine)}
    Hn = torch.tensor(host(clf.net.forward(X)).astype(np.float64), requires_grad=True)
    K, V, ptr, rows = Hn @ t["W_k"].T + t["b_k"], Hn @ t["W_v"].T + t["b_v"], host(g.graph_ptr), []
    for b in range(B):
        k, v = (a[ptr[b]:ptr[b + 1]].reshape(-1, heads, F // heads) for a in (K, V))
        alpha = torch.softmax(torch.einsum("shd,jhd->shj", t["P"].reshape(S, heads, -1), k) * (F // heads) ** -0.5, dim=2)
        rows.append(torch.einsum("shj,jhd->shd", alpha, v).reshape(1, S * F))
    ref = torch.cat(rows) @ t["W_c"].T + t["b_c"]
    K.retain_grad()
    (ref * torch.from_numpy(dlogits.astype(np.float64))).sum().backward()

    def close(got, want, what, size=None):
        want = want.detach().numpy()
        size = np.abs(want).max() if size is None else size
        frac = np.abs(host(got) - want).max() / (tol * size)
        print(f"{what}: worst |err| / bar = {frac:.4f}")
        assert size > 0 and frac <= 1, what
    close(clf.forward(X), ref, "logits")
    assert np.array_equal(host(clf.forward(X)), logits)
    for k, d in zip(names, dmine):   # db_k is zero in exact arithmetic (a softmax ignores a term shared by its keys): the size of its terms
        close(d, t[k].grad, "d" + k, float(K.grad.abs().sum(0).max()) if k == "b_k" else None)
    close(clf.net.grad_buffer(), Hn.grad, "dH")
    target = dev(env, (np.arange(B) % C).astype(np.int32))
    losses = [float(host(clf.train_step(X, target, 0.1))[0]) for _ in range(6)]
    assert losses[-1] < losses[0]
    g2 = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, t), k) for s, t, k in graphs[:2]])
    clf2, before = clf.on_batch(g2), host(clf.params()[-5]).copy()
    assert all(a is b for a, b in zip(clf2.params() + clf2.grads(), clf.params() + clf.grads()))
    clf2.train_step(X[:g2.n].contiguous(), target[:2].contiguous(), 0.1)
    assert not np.array_equal(host(clf.params()[-5]), before) and tuple(clf2.Z.shape) == (2, S * F)
