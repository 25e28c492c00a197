"""GPU tests of the dense segment attention calls on bf16 operands (run with -m gpu on an MI355X): ops.segment_attention / _bwd_rows /
_bwd_cols with torch.bfloat16 Q, K, V, G against tests/attn_ref.py on the all-pairs entry list.  The operands are float32 arrays rounded
to bf16 on the host; the float64 reference gets the SAME rounded values, so only the kernels' own arithmetic is measured.  LENGTHS and the
tile seams are tests/test_gpu_segment_attn.py's; the bars are tests/segment_attn_bf16_ref.py's.  Each test prints the worst fraction of its
bar.  Observed on an MI355X (worst over all cases): rowmax 0.18, rowsum 0.038, Y 0.0013, dot 0.28, dQ 0.0008, dK 0.0009, dV 0.0020.

With ONE bf16 term per weight operand the same tests gave Y 0.61, dQ 0.44, dK 0.47 and dV 1.0024 (test_backward[8x8] and [8x8-offset]
failed; a float64 emulation of the single rounding of alpha gave the same 1.0024325): one bf16 is good to 2^-8 relative, the bars allow
2^-9.  The kernels now give each weight as hi + lo, two bf16 terms; the bars are unchanged."""
import numpy as np
import pytest

from tests import attn_ref as ar
from tests import segment_attn_bf16_ref as br
from tests.test_gpu_attn import operands, padded, pads_kept
from tests.test_gpu_gat_fused import dev, env, held, host, per_feature  # noqa: F401 (env: the module fixture)
from tests.test_gpu_segment_attn import CASES, IDS, LENGTHS, SHAPES, seg  # noqa: F401 (seg: the module fixture)

pytestmark = pytest.mark.gpu


def rounded(H, D, n, qscale=1.0, values=None):
    o = operands(H, D, n, n, 0, False, values=values)
    o["Q"] *= np.float32(qscale)
    return {k: br.to_bf16(o[k]) for k in "QKVG"}


def half(env, a, bufs=None):
    """a (on bf16's grid) as a torch.bfloat16 device matrix; bufs: on a pitch of F + 3 one element off alignment between NaN pads"""
    t = dev(env, a).to(env["torch"].bfloat16)
    if bufs is None:
        return t
    rows, F = t.shape
    buf = t.new_full((rows * (F + 3) + 1,), float("nan"))
    view = buf[1:].view(rows, F + 3)[:, :F]
    view.copy_(t)
    bufs.append(buf)
    return view


@pytest.mark.parametrize("H,D", SHAPES)
def test_forward_exact(env, seg, H, D):
    """Q = 0, V from {-1, 0, 1}: every weight is 1, exact in bf16, so rowsum is the segment length, rowmax is 0 and Y =
    float32(sum) / float32(length) bit for bit: a dropped, doubled or foreign key fails it."""
    n, d = seg["n"], seg["d"]
    o = rounded(H, D, n, values=[-1.0, 0.0, 1.0])
    o["Q"][:] = 0
    Y, m, z = (host(t) for t in env["ops"].segment_attention(seg["ptr_d"], half(env, o["Q"]), half(env, o["K"]), half(env, o["V"]), H))
    total = np.add.reduceat(o["V"].astype(np.float64), seg["ptr"][:-1][np.diff(seg["ptr"]) > 0], axis=0)
    total = np.repeat(total, [k for k in LENGTHS if k], axis=0)
    assert np.array_equal(z, np.repeat(d[:, None], H, 1).astype(np.float32)) and np.all(m == 0)
    assert np.array_equal(Y, total.astype(np.float32) / d[:, None].astype(np.float32))


@pytest.mark.parametrize("H,D,offset,qscale", CASES, ids=IDS)
def test_forward(env, seg, H, D, offset, qscale):
    """General data; qscale = 60: the maximum rises in a later streamed tile of the 200-row segment (asserted on the rounded operands).
    offset: every matrix off alignment between NaN pads that must survive -- the 2-byte copy path and the scalar stores.  A mismatch
    between the weights' register order and the transposed image's row order is an O(1) error in Y."""
    n, d, F = seg["n"], seg["d"], H * D
    o = rounded(H, D, n, qscale)
    scale = float(np.float32(D ** -0.5))
    lo, hi = seg["big"]
    assert ((o["Q"][lo:hi, :D].astype(np.float64) @ o["K"][lo:hi, :D].astype(np.float64).T).argmax(1) >= 32).any()
    bufs = [] if offset else None
    Y, m, z = (host(t) for t in env["ops"].segment_attention(seg["ptr_d"], *(half(env, o[k], bufs) for k in "QKV"), H, scale=scale,
                                                            out=padded(dev(env, np.zeros((n, F), np.float32)), bufs) if offset else None))
    assert (not offset or pads_kept(bufs, F)) and np.all(np.isfinite(Y))
    ref = ar.forward(seg["qi"], seg["ki"], None, n, o["Q"], o["K"], o["V"], None, H, scale)
    held(m, ref["m"], br.c_s(D), ref["S_m"], "rowmax")
    held(z, ref["z"], per_feature(br.c_z(d, D), n), ref["S_z"], "rowsum")
    held(Y, ref["Y"], per_feature(br.c_Y(d, D), n), ref["S_Y"], "Y")


@pytest.mark.parametrize("H,D,offset,beta", [c[:3] + (0.0,) for c in CASES[:-1]] + [(8, 8, False, 1.0)], ids=IDS[:-1] + ["8x8-beta1"])
def test_backward(env, seg, H, D, offset, beta):
    """dot, dQ, dK, dV from the float32-rounded m, z, Y (and, column side, dot) of the reference; G is bf16 on both sides.  beta = 1 adds
    onto a given dK / dV."""
    ops = env["ops"]
    n, d, F = seg["n"], seg["d"], H * D
    scale = float(np.float32(D ** -0.5))
    o = rounded(H, D, n)
    fw = ar.forward(seg["qi"], seg["ki"], None, n, o["Q"], o["K"], o["V"], None, H, scale)
    Y, m, z = (fw[k].astype(np.float32) for k in ("Y", "m", "z"))
    ref = ar.backward(seg["qi"], seg["ki"], None, n, n, o["G"], o["Q"], o["K"], o["V"], None, H, scale, m, z, Y=Y)
    bufs = [] if offset else None
    wrap = (lambda t: padded(t, bufs)) if offset else (lambda t: t)
    G, Q, K, V = (half(env, o[k], bufs) for k in "GQKV")
    old = np.random.default_rng(H).uniform(-1, 1, (3, n, F)).astype(np.float32)
    stats = (dev(env, m), dev(env, z))
    dQ, dot = ops.segment_attention_bwd_rows(seg["ptr_d"], G, Q, K, V, wrap(dev(env, Y)), H, *stats, scale=scale, dq_out=wrap(dev(env, old[2])))
    dK, dV = ops.segment_attention_bwd_cols(seg["ptr_d"], G, Q, K, V, H, *stats, dev(env, ref["dot"].astype(np.float32)), scale=scale,
                                            dk_out=wrap(dev(env, old[0])), dv_out=wrap(dev(env, old[1])), beta=beta)
    assert not offset or pads_kept(bufs, F)
    held(host(dot), ref["dot"], br.c_dot(D), ref["S_dot"], "dot")
    held(host(dQ), ref["dQ"], per_feature(br.c_dQ(d, D), n), ref["S_dQ"], "dQ")
    held(host(dK), ref["dK"] + beta * old[0], per_feature(br.c_dK(d, D), n), ref["S_dK"] + beta * np.abs(old[0]), "dK")
    held(host(dV), ref["dV"] + beta * old[1], per_feature(br.c_dV(d, D), n), ref["S_dV"] + beta * np.abs(old[1]), "dV")
