"""GPU tests of the fused epilogues of gemm_dma_kernel (csrc/gnnx_gemm.hip; run with -m gpu on an MI355X): the four entry points
the training step and the sharded step call -- gnnx_gemm_relu_colsum_f32, gnnx_gemm_bn_stats_f32, gnnx_gemm_nt_bf16out_f32 and
gnnx_gemm_nt_rows_to_slots_f32 -- on every geometry (256 x 256, 256 x 128, the guarded last column tile), with whole tiles, a 255-row
and a 1-row tail, more than one M-tile per workgroup (the carried column sums), every decline to the separate passes, and every
operand a view inside a NaN-filled buffer.  The case table, the float64 references and the comparisons are tests/gemm_fused_ref.py;
tests/test_gemm_fused_ref_cpu.py proves that the table reaches every cell and that each comparison rejects a wrong kernel.

Legs (none restates a summation order):
  exact     operands from {-1, 0, 1}: C / H equal the float64 product on every element; the column sums EQUAL the float64 sums (the
            reference asserts sum|term| < 2^24 per column first, so the float32 sums have one right value in any order); the
            BatchNorm mean within one float32 ulp and the variance within 2^-23 var + 2^-50 Q / M of float64 where the fused kernel
            ran, at the bars of tests/test_gpu_norm.py where the call falls back.
  mask      Y cycles through +0, -0, +-denormal, FLT_MIN, NaN, +-inf, +-1 in fused tiles and in the ragged tail: kept where IEEE
            Y > 0, in the fused epilogue and in the three-pass fallback alike.
  poison    rows of A whose products are +-inf and NaN under a mask <= 0: +0 in C, nothing in the sums (select, not multiply).
  rounding  uniform operands: C bit-equal to ops.gemm + torch.where, colsum within 1e-5 * max(1, sum|C|) of float64.
  offset    uniform X + 3 and X - 20: the single-pass variance against float64 at gemm_fused_ref.offset_var_rtol (8 x the measured error).
  bf16      one-hot X against the bfloat16 special values: ties, overflow to inf, denormals, -0 and NaN through the epilogue's cast.
  slots     H and the send buffer of the pack epilogue against rows_to_slots_ref, sentinel rows included."""
import ctypes
import importlib
import time

import numpy as np
import pytest

from tests import gemm_fused_ref as R
from tests.helpers import embed, holds_fill
from tests.norm_ref import assert_bits, check_exact, gamma_k

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -12345.0
T0 = time.time()


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    yield dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))
    print(f"\ntests/test_gpu_gemm_fused.py: {time.time() - T0:.1f} s from import to the last test")


def up(env, a, mode="a", fill=NAN):
    """(buffer, view) of helpers.embed holding the host array `a` (None: the view keeps the fill -- an output)."""
    rows, cols = a if isinstance(a, tuple) else a.shape
    buf, view = embed(env, rows, cols, mode, fill)
    if not isinstance(a, tuple) and view.numel():
        view.copy_(env["torch"].from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(env["dev"]))
    return buf, view


def vec_out(env, n, fill=NAN):
    """(buffer, view): an [n] output 4 elements into a filled buffer of n + 8."""
    buf = env["torch"].full((n + 8,), fill, dtype=env["torch"].float32, device=env["dev"])
    return buf, buf[4:4 + n]


def host(t):
    return t.detach().cpu().numpy()


def check_fill(bufs, view_of, what):
    """Every buffer holds its fill outside the view: the views are overwritten with the fill, then the whole buffer is checked."""
    for name, buf in bufs.items():
        if name in view_of:
            view_of[name].fill_(NAN)
        assert holds_fill(buf, NAN), f"{what}: the {name} buffer changed outside its view"


# ------------------------------------------------------------------ 1. gnnx_gemm_relu_colsum_f32
def relu_call(env, d, layout):
    """One call on fresh embedded operands; returns (C host, colsum host, buffers, views)."""
    bufs, views = {}, {}
    for name, mode, a in (("A", layout[0], d["A"]), ("B", layout[1], d["B"]), ("C", layout[2], d["Y"].shape), ("Y", layout[3], d["Y"])):
        bufs[name], views[name] = up(env, a, mode)
    bufs["colsum"], views["colsum"] = vec_out(env, d["Y"].shape[1])
    env["ops"].gemm_relu_colsum(views["A"], views["B"], views["Y"], out=views["C"], colsum_out=views["colsum"])
    return host(views["C"]), host(views["colsum"]), bufs, views


@pytest.mark.parametrize("case", R.RELU_CASES, ids=R.case_id)
def test_relu_colsum_exact_mask_and_poison_legs(env, case):
    data = R.relu_data(case.M, case.N, case.K)               # asserts the exactness condition of all three legs
    for leg in ("exact", "mask", "poison"):
        d = data[leg]
        what = f"{case.name} {leg} leg (fused rows {R.fused_rows(case.M, case.N, case.K, R.relu_aligned(case))})"
        C, colsum, bufs, views = relu_call(env, d, case.layout)
        R.check_relu_colsum(C, colsum, d, what)
        if leg == "exact":
            C2, colsum2, _, _ = relu_call(env, d, case.layout)
            assert_bits(C2, C, what + ": second call C")
            assert_bits(colsum2, colsum, what + ": second call colsum")
        # the inputs are unchanged, and nothing outside a view was written
        for name in ("A", "B", "Y"):
            assert_bits(host(views[name]), d[name], f"{what}: input {name}")
        check_fill(bufs, views, what)


def test_relu_colsum_of_no_rows_is_zero(env):
    c = R.RELU_EMPTY
    d = dict(A=np.zeros((0, c.K), np.float32), B=R.int_matrix(c.K, c.N, 1), Y=np.zeros((0, c.N), np.float32))
    _, colsum, bufs, views = relu_call(env, d, c.layout)
    assert_bits(colsum, np.zeros(c.N, np.float32), "M == 0: colsum")
    check_fill(bufs, {"colsum": views["colsum"], "B": views["B"]}, "M == 0")


@pytest.mark.parametrize("case", R.RELU_CASES, ids=R.case_id)
def test_relu_colsum_rounding_leg(env, case):
    ops, torch = env["ops"], env["torch"]
    M, N, K = case.M, case.N, case.K
    _, A = up(env, (M, K), case.layout[0])
    _, B = up(env, (K, N), case.layout[1])
    _, Y = up(env, (M, N), case.layout[3])
    _, C = up(env, (M, N), case.layout[2])
    A.copy_(ops.uniform_pm1(81, (M, K), device=env["dev"]))
    B.copy_(ops.uniform_pm1(82, (K, N), scale=K ** -0.5, device=env["dev"]))
    Y.copy_(torch.relu(ops.uniform_pm1(83, (M, N), device=env["dev"])))
    _, colsum = vec_out(env, N)
    ops.gemm_relu_colsum(A, B, Y, out=C, colsum_out=colsum)
    ref = ops.gemm(A, B)
    ref = torch.where(Y > 0, ref, torch.zeros_like(ref))
    assert torch.equal(C, ref), f"{case.name}: masked product differs from gemm + where in {int((C != ref).sum())} elements"
    R.check_colsum_rounding(host(colsum), host(ref), case.name)


# ------------------------------------------------------------------ 2. gnnx_gemm_bn_stats_f32
def bn_call(env, X, W, layout, N):
    """The entry point through the C ABI on embedded operands (layout[3] == "o": the workspace pointer moved up by 4 bytes).
    Returns (H view, mean host, var host, buffers, views)."""
    ops, capi = env["ops"], env["capi"]
    M, K = X.shape
    bufs, views = {}, {}
    for name, mode, a in (("X", layout[0], X), ("W", layout[1], W), ("H", layout[2], (M, N))):
        bufs[name], views[name] = up(env, a, mode)
    for name in ("mean", "var"):
        bufs[name], views[name] = vec_out(env, N)
    wsb = ctypes.c_size_t(0)
    capi.call("gnnx_gemm_bn_stats_workspace", M, N, K, ctypes.byref(wsb))
    off = 4 if layout[3] == "o" else 0
    ws = ops._workspace(wsb.value + 16, env["dev"], "gemm_fused_test")
    assert ws.data_ptr() % 16 == 0
    capi.call("gnnx_gemm_bn_stats_f32", M, N, K, ops._ptr(views["X"]), views["X"].stride(0), ops._ptr(views["W"]), views["W"].stride(0),
              ops._ptr(views["H"]), views["H"].stride(0), ops._ptr(views["mean"]), ops._ptr(views["var"]),
              ctypes.c_void_p(ws.data_ptr() + off), wsb.value + 16 - off, ops._stream())
    return views["H"], host(views["mean"]), host(views["var"]), bufs, views


@pytest.mark.parametrize("case", R.BN_CASES, ids=R.case_id)
def test_bn_stats_exact_leg(env, case):
    ops = env["ops"]
    M, N, K = case.M, case.N, case.K
    ref = R.bn_data(M, N, K)                                  # asserts the exactness condition
    rows = R.fused_rows(M, N, K, R.bn_aligned(case))
    what = f"{case.name} (fused rows {rows})"
    H, mean, var, bufs, views = bn_call(env, ref["X"], ref["W"], case.layout, N)
    assert_bits(host(H), ref["H"].astype(np.float32), what + ": H")
    assert env["torch"].equal(H, ops.linear_fwd(views["X"], views["W"])), what + ": H differs from linear_fwd"
    if rows:
        R.check_bn_fused(mean, var, ref, what)
    else:
        # the exact pair of calls, at the bars of tests/test_gpu_norm.py: the mean is float32(sum) * (1 / n) on exact sums, the variance
        # is bn_partial's bits on that mean and inside gamma_(n + 3) * sum|term| / n of float64
        check_exact(ref["H"], 1.0)
        inv_n = np.float32(1) / np.float32(M)
        assert_bits(mean, ref["H"].sum(0).astype(np.float32) * inv_n, what + ": fallback mean")
        assert_bits(var, host(ops.bn_partial(H, views["mean"], float(inv_n))), what + ": fallback var vs bn_partial on its mean")
        terms = (ref["H"] - mean.astype(np.float64)) ** 2
        err, bound = np.abs(var - terms.sum(0) / M), gamma_k(M + 3) * terms.sum(0) / M
        assert (err <= bound).all(), f"{what}: fallback var err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}"
    assert var[N // 3] == 0.0 and not np.signbit(var[N // 3]), what + ": the variance of the constant column"
    for name in ("X", "W"):
        assert_bits(host(views[name]), ref[name], f"{what}: input {name}")
    check_fill(bufs, views, what)


@pytest.mark.parametrize("M,N,K,offset", R.OFFSET_CASES, ids=lambda v: str(v))
def test_bn_stats_offset_leg(env, M, N, K, offset):
    ops = env["ops"]
    X, W = R.offset_operands(M, N, K, offset)
    H, mean, var, _, views = bn_call(env, X, W, "aaaa", N)
    assert R.fused_rows(M, N, K) == 2048
    assert env["torch"].equal(H, ops.linear_fwd(views["X"], views["W"])), "H differs from linear_fwd"
    em, ev = R.offset_errors(mean, var, host(H))
    print(f"\noffset leg {M}x{N}x{K} offset {offset:+.1f}: mean err / bound = {em:.4f}, largest relative variance error = {ev:.3e}")
    R.check_bn_offset(mean, var, host(H), R.offset_var_rtol(M, N, K, offset), f"{M}x{N}x{K} offset {offset}")


# ------------------------------------------------------------------ 3. gnnx_gemm_nt_bf16out_f32
@pytest.mark.parametrize("M,N,K", R.BF16_SHAPES, ids=lambda v: str(v))
def test_bf16_output_special_values(env, M, N, K):
    ops, torch = env["ops"], env["torch"]
    ref = R.bf16_data(M, N, K)
    assert R.fused_rows_bf16(M, N, K) == 2048 < M
    _, X = up(env, ref["X"])
    _, W = up(env, ref["W"])
    assert_bits(host(W), ref["W"], "W upload keeps every bit pattern")
    buf = torch.full((M + 6, N + 16), NAN, dtype=torch.bfloat16, device=env["dev"])     # N = 100: rows on the 8-byte grid only
    out = buf[4:4 + M, 8:8 + N]
    assert out.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0 and out.stride(0) > N
    got = ops.linear_fwd_bf16(X, W, out=out)
    assert got.data_ptr() == out.data_ptr()
    R.check_bf16(host(out.view(torch.int16)), ref, f"{M}x{N}x{K}")
    two = ops.to_bf16(ops.gemm(X, W, transB=True))
    keep = torch.from_numpy(ref["keep"]).to(env["dev"])
    assert torch.equal(out.view(torch.int16)[:, keep], two.view(torch.int16)[:, keep]), "differs from gemm followed by to_bf16"
    assert bool(two[:, ref["nan_col"]].isnan().all())
    out.fill_(NAN)
    assert bool(buf.isnan().all()), "the bf16 buffer changed outside the column slice"


# ------------------------------------------------------------------ 4. gnnx_gemm_nt_rows_to_slots_f32
@pytest.mark.parametrize("M,N,K", R.SLOT_SHAPES, ids=lambda v: str(v))
def test_slot_pack_epilogue(env, M, N, K):
    ops, torch = env["ops"], env["torch"]
    ref = R.slot_data(M, N, K, SENTINEL)
    _, X = up(env, ref["X"])
    _, W = up(env, ref["W"])
    Hbuf, H = up(env, (M, N))
    sbuf, send = embed(env, ref["n_slots"], N, "a", SENTINEL)
    assert H.stride(0) > N and send.stride(0) > N
    table = torch.from_numpy(ref["table"]).to(env["dev"])
    ops.linear_fwd_rows_to_slots(X, W, H, table, send)
    what = f"{M}x{N}x{K} (fused rows {R.fused_rows_slots(M, N, K)})"
    assert_bits(host(H), ref["H"].astype(np.float32), what + ": H")
    assert_bits(host(send), ref["send"], what + ": send")
    assert (ref["send"][-R.SLOT_SPARE:] == SENTINEL).all()
    H.fill_(NAN)
    send.fill_(SENTINEL)
    assert holds_fill(Hbuf, NAN) and holds_fill(sbuf, SENTINEL), what + ": wrote outside H or send"


# ------------------------------------------------------------------ 5. statuses
INVALID, SHAPE, WORKSPACE = -1, -2, -4


def test_refusals_give_the_header_codes_and_write_nothing(env):
    """Through the C ABI: a workspace one byte short (GNNX_ERR_WORKSPACE), a null operand, a leading dimension one below its minimum,
    N = 0, K = 0 (GNNX_ERR_INVALID_ARG), and M = 2047 for the bf16 entry (GNNX_ERR_SHAPE).  Every output is pre-filled and untouched."""
    ops, capi, torch, dev = env["ops"], env["capi"], env["torch"], env["dev"]
    L = capi.lib()
    M, N, K = 2303, 128, 64
    f = lambda *shape: torch.full(shape, 1.0, dtype=torch.float32, device=dev)     # noqa: E731
    s = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)     # noqa: E731
    A, B, Y, X, W = f(M, K), f(K, N), f(M, N), f(M, K), f(N, K)
    C, colsum, mean, var, send = s(M, N), s(N), s(N), s(N), s(40, N)
    Hb = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=dev)
    table = torch.full((M, 8), -1, dtype=torch.int32, device=dev)
    table[:40, 0] = torch.arange(40, dtype=torch.int32, device=dev)
    outputs = (C, colsum, mean, var, send, Hb)

    def need(name):
        b = ctypes.c_size_t(0)
        capi.call(name, M, N, K, ctypes.byref(b))
        return b.value

    p, st = ops._ptr, ops._stream()

    def relu(M=M, N=N, K=K, A=A, B=B, Y=Y, C=C, colsum=colsum, lda=K, ldb=N, ldy=N, ldc=N, short=0):
        nb = need("gnnx_gemm_relu_colsum_workspace")
        return L.gnnx_gemm_relu_colsum_f32(M, N, K, p(A), lda, p(B), ldb, p(Y), ldy, p(C), ldc, p(colsum), p(ops._workspace(nb, dev, "t")), nb - short, st)

    def bn(M=M, N=N, K=K, X=X, W=W, H=C, mean=mean, var=var, ldx=K, ldw=K, ldh=N, short=0):
        nb = need("gnnx_gemm_bn_stats_workspace")
        return L.gnnx_gemm_bn_stats_f32(M, N, K, p(X), ldx, p(W), ldw, p(H), ldh, p(mean), p(var), p(ops._workspace(nb, dev, "t")), nb - short, st)

    def bf16(M=M, N=N, K=K, X=X, W=W, H=Hb, ldx=K, ldw=K, ldh=N, short=0):
        nb = need("gnnx_gemm_nt_bf16out_workspace")
        return L.gnnx_gemm_nt_bf16out_f32(M, N, K, p(X), ldx, p(W), ldw, p(H), ldh, p(ops._workspace(nb, dev, "t")), nb - short, st)

    def slots(M=M, N=N, K=K, X=X, W=W, H=C, table=table, send=send, ldx=K, ldw=K, ldh=N, lds=N, short=0):
        nb = need("gnnx_gemm_nt_rows_to_slots_workspace")
        return L.gnnx_gemm_nt_rows_to_slots_f32(M, N, K, p(X), ldx, p(W), ldw, p(H), ldh, p(table), p(send), lds, p(ops._workspace(nb, dev, "t")), nb - short, st)

    entries = {relu: (("A", "B", "Y", "C", "colsum"), (("lda", K), ("ldb", N), ("ldy", N), ("ldc", N))),
               bn: (("X", "W", "H", "mean", "var"), (("ldx", K), ("ldw", K), ("ldh", N))),
               bf16: (("X", "W", "H"), (("ldx", K), ("ldw", K), ("ldh", N))),
               slots: (("X", "W", "H", "table", "send"), (("ldx", K), ("ldw", K), ("ldh", N), ("lds", N)))}
    for fn, (operands, lds) in entries.items():
        assert fn(short=1) == WORKSPACE, f"{fn.__name__}: workspace one byte short"
        for name in operands:
            assert fn(**{name: None}) == INVALID, f"{fn.__name__}: null {name}"
        for name, least in lds:
            assert fn(**{name: least - 1}) == INVALID, f"{fn.__name__}: {name} = {least - 1}"
        assert fn(N=0) == INVALID and fn(K=0) == INVALID, f"{fn.__name__}: N = 0 or K = 0"
    assert bf16(M=2047) == SHAPE
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t == SENTINEL).all()), "a refused call wrote to an output"
    for fn in entries:                                        # and the same arguments, unrefused, succeed
        assert fn() == 0, f"{fn.__name__}: {L.gnnx_last_error().decode()}"
    torch.cuda.synchronize()
