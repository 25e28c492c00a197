"""GPU tests of the dense segment attention calls (run with -m gpu on an MI355X): ops.segment_attention / _bwd_rows / _bwd_cols and
TransformerStack(global_attention=True) against tests/attn_ref.py on the all-pairs entry list (tests/segment_attn_ref.py derives c).

The kernels' tiles are 32 own rows x 32 streamed rows.  LENGTHS, from row 0: an empty first segment; 1, 1, 3 and the head of 31 share
tile 0 (four segments in one tile); 31 and 32 start and end mid-tile; 33, 64, 65 are one tile + 1, two tiles, two tiles + 1 of streamed
rows; an empty segment in the middle; 5 and 2 lie inside one tile; 200 is seven streamed tiles and eight own tiles; 96 ends the batch at
533 rows = 16 tiles + 21 (a last partial tile).  Each test prints the worst fraction of its bar.  Observed on an MI355X (worst over all
cases): rowmax 0.28, rowsum 0.033, Y 0.011, dot 0.27, dQ 0.010, dK 0.0095, dV 0.021."""
import numpy as np
import pytest

from tests import attn_ref as ar
from tests import segment_attn_ref as sr
from tests.test_gpu_attn import close, operands, padded, pads_kept
from tests.test_gpu_gat_fused import dev, env, held, host, per_feature  # noqa: F401 (env: the module fixture)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 1, 3, 31, 32, 33, 0, 64, 65, 5, 200, 2, 96]
SHAPES = [(1, 64), (8, 8), (4, 6), (2, 128), (3, 20)]   # (4, 6): scalar loads; (3, 20): a padded D with D % 4 == 0


@pytest.fixture(scope="module")
def seg(env):
    ptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    qi, ki, d = sr.pairs(ptr)
    return dict(ptr=ptr, ptr_d=dev(env, ptr), qi=qi, ki=ki, d=d, n=int(ptr[-1]), big=(int(ptr[11]), int(ptr[12])))


@pytest.mark.parametrize("H,D", SHAPES)
def test_forward_exact(env, seg, H, D):
    """Q = 0: every score is +0, so rowsum is the segment length and Y = float32(sum) / float32(length) bit for bit in any order: a
    dropped, doubled or wrongly masked key, or a key of the neighbouring segment, fails it."""
    n, d = seg["n"], seg["d"]
    o = operands(H, D, n, n, 0, False, values=[-1.0, 0.0, 1.0])
    o["Q"][:] = 0
    Y, m, z = (host(t) for t in env["ops"].segment_attention(seg["ptr_d"], dev(env, o["Q"]), dev(env, o["K"]), dev(env, o["V"]), H))
    total = np.add.reduceat(o["V"].astype(np.float64), seg["ptr"][:-1][np.diff(seg["ptr"]) > 0], axis=0)
    total = np.repeat(total, [k for k in LENGTHS if k], axis=0)
    assert np.array_equal(z, np.repeat(d[:, None], H, 1).astype(np.float32)) and np.all(m == 0)
    assert np.array_equal(Y, total.astype(np.float32) / d[:, None].astype(np.float32))


CASES = [(h, d, False, 1.0) for h, d in SHAPES] + [(8, 8, True, 1.0), (8, 8, False, 60.0)]
IDS = [f"{h}x{d}{'-offset' * o}{'-q60' * (q > 1)}" for h, d, o, q in CASES]


@pytest.mark.parametrize("H,D,offset,qscale", CASES, ids=IDS)
def test_forward(env, seg, H, D, offset, qscale):
    """General data; qscale = 60: expf overflows unless the maximum is subtracted, and on the 200-row segment the maximum rises in a later
    streamed tile.  offset: every matrix on a pitch of F + 3 at a base 4 bytes off alignment, between NaN pads that must survive."""
    n, d, F = seg["n"], seg["d"], H * D
    o = operands(H, D, n, n, 0, False)
    o["Q"] *= np.float32(qscale)
    scale = float(np.float32(D ** -0.5))
    lo, hi = seg["big"]
    assert ((o["Q"][lo:hi, :D].astype(np.float64) @ o["K"][lo:hi, :D].astype(np.float64).T).argmax(1) >= 32).any()
    bufs = []
    wrap = (lambda t: padded(t, bufs)) if offset else (lambda t: t)
    Y, m, z = (host(t) for t in env["ops"].segment_attention(seg["ptr_d"], *(wrap(dev(env, o[k])) for k in "QKV"), H, scale=scale,
                                                            out=wrap(dev(env, np.zeros((n, F), np.float32))) if offset else None))
    assert pads_kept(bufs, F) and np.all(np.isfinite(Y))
    ref = ar.forward(seg["qi"], seg["ki"], None, n, o["Q"], o["K"], o["V"], None, H, scale)
    held(m, ref["m"], sr.c_s(D), ref["S_m"], "rowmax")
    held(z, ref["z"], per_feature(sr.c_z(d, D), n), ref["S_z"], "rowsum")
    held(Y, ref["Y"], per_feature(sr.c_Y(d, D), n), ref["S_Y"], "Y")


@pytest.mark.parametrize("H,D,offset,beta", [c[:3] + (0.0,) for c in CASES[:-1]] + [(8, 8, False, 1.0)], ids=IDS[:-1] + ["8x8-beta1"])
def test_backward(env, seg, H, D, offset, beta):
    """dot, dQ, dK, dV from the float32-rounded m, z, Y (and, column side, dot) of the reference.  beta = 1 adds onto a given dK / dV."""
    ops = env["ops"]
    n, d, F = seg["n"], seg["d"], H * D
    scale = float(np.float32(D ** -0.5))
    o = operands(H, D, n, n, 0, False)
    fw = ar.forward(seg["qi"], seg["ki"], None, n, o["Q"], o["K"], o["V"], None, H, scale)
    Y, m, z = (fw[k].astype(np.float32) for k in ("Y", "m", "z"))
    ref = ar.backward(seg["qi"], seg["ki"], None, n, n, o["G"], o["Q"], o["K"], o["V"], None, H, scale, m, z, Y=Y)
    bufs = []
    wrap = (lambda t: padded(t, bufs)) if offset else (lambda t: t)
    G, Q, K, V = (wrap(dev(env, o[k])) for k in "GQKV")
    old = np.random.default_rng(H).uniform(-1, 1, (3, n, F)).astype(np.float32)
    stats = (dev(env, m), dev(env, z))
    dQ, dot = ops.segment_attention_bwd_rows(seg["ptr_d"], G, Q, K, V, wrap(dev(env, Y)), H, *stats, scale=scale, dq_out=wrap(dev(env, old[2])))
    dK, dV = ops.segment_attention_bwd_cols(seg["ptr_d"], G, Q, K, V, H, *stats, dev(env, ref["dot"].astype(np.float32)), scale=scale,
                                            dk_out=wrap(dev(env, old[0])), dv_out=wrap(dev(env, old[1])), beta=beta)
    assert pads_kept(bufs, F)
    held(host(dot), ref["dot"], sr.c_dot(D), ref["S_dot"], "dot")
    held(host(dQ), ref["dQ"], per_feature(sr.c_dQ(d, D), n), ref["S_dQ"], "dQ")
    held(host(dK), ref["dK"] + beta * old[0], per_feature(sr.c_dK(d, D), n), ref["S_dK"] + beta * np.abs(old[0]), "dK")
    held(host(dV), ref["dV"] + beta * old[1], per_feature(sr.c_dV(d, D), n), ref["S_dV"] + beta * np.abs(old[1]), "dV")


def test_transformer_stack_global(env):
    """One training step (lr = 0) of a two-layer stack with the global branch on a batch of five small graphs against float64 autograd, at
    the bars of tests/test_gpu_attn.py::test_stack_step_vs_float64; without the option the parameter shapes are the old ones."""
    ops, torch = env["ops"], env["torch"]
    sizes, dims, heads = [5, 40, 1, 33, 17], [12, 16, 6], [2, 1]
    rng = np.random.default_rng(7)
    graphs = [(rng.integers(0, k, 3 * k).astype(np.int32), rng.integers(0, k, 3 * k).astype(np.int32), k) for k in sizes]
    g = ops.GraphBatch.from_graphs([(dev(env, s), dev(env, t), k) for s, t, k in graphs])
    n = g.n
    X = rng.uniform(-1, 1, (n, dims[0])).astype(np.float32)
    target, rows = (np.arange(n) % dims[-1]).astype(np.int32), np.arange(0, n, 2, dtype=np.int32)
    assert [tuple(w.shape) for w in ops.TransformerStack(g, dims, heads=heads, seed=3).W] == [(64, 12), (24, 16)]
    net = ops.TransformerStack(g, dims, heads=heads, global_attention=True, seed=3)
    assert [tuple(w.shape) for w in net.W] == [(112, 12), (42, 16)]
    for l in range(2):
        net.b[l].copy_(dev(env, rng.uniform(-0.2, 0.2, dims[l + 1]).astype(np.float32)))
    P = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in ("W", "b")}
    loss = net.train_step(dev(env, X), dev(env, target), dev(env, rows), lr=0.0)
    logits = host(net.forward(dev(env, X)))

    def attend(Q, K, V, qi, ki, Hh):
        D = Q.shape[1] // Hh
        s = (Q[qi] * K[ki]).reshape(-1, Hh, D).sum(2) * D ** -0.5
        x = torch.exp(s - torch.full((n, Hh), -np.inf, dtype=torch.float64).scatter_reduce(0, qi[:, None].expand(-1, Hh), s.detach(), "amax")[qi])
        alpha = x / torch.zeros((n, Hh), dtype=torch.float64).index_add(0, qi, x)[qi]
        return torch.zeros_like(Q).index_add(0, qi, alpha.repeat_interleave(D, 1) * V[ki])
    rp = host(g.rowptr)
    local = (torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(host(g.colidx).astype(np.int64)))
    glob = tuple(torch.from_numpy(a) for a in sr.pairs(host(g.graph_ptr))[:2])
    h = torch.from_numpy(X.astype(np.float64))
    for l, Hh in enumerate(heads):
        Q, K, V, S, Qg, Kg, Vg = (h @ P["W"][l].T).split(dims[l + 1], dim=1)
        Z = attend(Q, K, V, *local, Hh) + attend(Qg, Kg, Vg, *glob, Hh) + S + P["b"][l]
        h = torch.relu(Z) if l == 0 else Z
    zr = h[torch.from_numpy(rows.astype(np.int64))]
    picked = zr[torch.arange(len(rows)), torch.from_numpy(target.astype(np.int64))[rows]]
    ref = (-torch.log(torch.exp(picked) / (torch.exp(zr).sum(1) + 1e-20))).sum() / len(rows)
    ref.backward()
    assert abs(float(host(loss)[0]) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach())))
    assert close(logits, h.detach().numpy())
    for k in ("W", "b"):
        for l in range(2):
            r = P[k][l].grad.numpy()
            assert np.abs(r).max() > 0 and close(host(getattr(net, "d" + k)[l]), r), f"d{k}{l}"
