"""GPU tests of gnnx_gemm_f32's stated contract (include/gnnx.h; run with -m gpu on an MI355X): C = alpha * op(A) . op(B) + beta * C
for "any shape, any transposition", and "which kernel ran never changes a bit" -- on every dispatch cell of csrc/gnnx_gemm.hip.  The
shape table is tests/gemm_ref.CASES; tests/test_gemm_contract_cpu.py proves from the restated dispatch that it reaches every cell.

Every operand of every leg is a VIEW inside a larger buffer filled with NaN (the exact leg once more with +Inf): rows before and
after, columns left and right, a pitch wider than the width; with beta == 0 the C view itself is pre-filled.  A mask done by
multiplication, a read of the padding between width and pitch, or a read of C that beta == 0 forbids shows as a NaN in the result.

Legs (none restates a summation order):
  exact     {-1, 0, 1} operands, small-integer C0, alpha in {1, 2, -0.5}, beta in {0, 1, -1, 0.5}: every partial sum is an integer
            below 2^24 and every scaling exact, so the result EQUALS alpha * (A64 @ B64) + beta * C0 in float64 on every element in
            any summation order; the C buffer outside the view still holds the fill.
  rounding  uniform operands, alpha = 0.3, beta = -1.7 (0 where the path needs it) against float64 at the project's bar,
            1e-5 * max(1, |ref|, absum), absum = |alpha| (|A| @ |B|) + |beta| |C0| (helpers.assert_rows_close).
  identity  with P the same call at alpha = 1, beta = 0: the result at (alpha, beta) equals gemm_ref.epilogue_f32(P, C0, alpha, beta)
            bit for bit -- one epilogue arithmetic in every kernel.
  chain     a case served by more than one kernel or by a non-generic one: 1000-row slices (row 0, across a tile seam, the tail)
            recomputed as short products equal the tall result bit for bit, at alpha = 2; split-K: two runs give the same bits."""
import importlib
import zlib

import numpy as np
import pytest

from tests import gemm_ref as gr
from tests.helpers import ROWS_AFTER, ROWS_BEFORE, assert_rows_close, embed, fill_small_ints, holds_fill  # noqa: F401

pytestmark = pytest.mark.gpu

FILLS = {"nan": float("nan"), "inf": float("inf")}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def operand_shapes(case):
    a = (case.K, case.M) if case.trans[0] == "T" else (case.M, case.K)
    b = (case.N, case.K) if case.trans[1] == "T" else (case.K, case.N)
    return a, b


def op(t, transposed):
    return t.t() if transposed else t


def product64(case, A, B):
    return op(A.double(), case.trans[0] == "T") @ op(B.double(), case.trans[1] == "T")


def status_of(env, case, A, B, Cv, alpha, beta, M=None, ws_bytes=None, lda=None, ldb=None, ldc=None):
    """gnnx_gemm_f32 through the C ABI, returning its status.  ws_bytes None: what gnnx_gemm_workspace asks for this M (0 for a case
    that runs without workspace)."""
    ops, capi = env["ops"], env["capi"]
    tA, tB = int(case.trans[0] == "T"), int(case.trans[1] == "T")
    M = case.M if M is None else M
    if ws_bytes is None:
        ws_bytes = 0 if case.ws == "zero" else capi.gemm_workspace(tA, tB, M, case.N, case.K)
    ws = ops._workspace(ws_bytes, env["dev"], "gemm_contract") if ws_bytes else None
    ptr = lambda t: ops._ptr(t) if t is not None and t.numel() else None   # noqa: E731  (an empty operand: K = 0 takes null)
    return capi.lib().gnnx_gemm_f32(tA, tB, M, case.N, case.K, float(alpha), ptr(A), A.stride(0) if lda is None else lda, ptr(B),
                                    B.stride(0) if ldb is None else ldb, float(beta), ptr(Cv), Cv.stride(0) if ldc is None else ldc,
                                    ptr(ws), ws_bytes, ops._stream())


def run(env, case, A, B, Cv, alpha, beta, **kw):
    st = status_of(env, case, A, B, Cv, alpha, beta, **kw)
    assert st == 0, f"{case.name}: status {st}: {env['capi'].lib().gnnx_last_error().decode()}"
    return Cv


def int_operands(env, case, fill):
    torch = env["torch"]
    gen = torch.Generator(device=env["dev"])
    gen.manual_seed(zlib.crc32(case.name.encode()))
    (ar, ac), (br, bc) = operand_shapes(case)
    _, A = embed(env, ar, ac, case.layout[0], fill)
    _, B = embed(env, br, bc, case.layout[1], fill)
    fill_small_ints(A, gen)
    fill_small_ints(B, gen)
    C0 = fill_small_ints(torch.empty((case.M, case.N), dtype=torch.float32, device=env["dev"]), gen, -3, 3)
    return A, B, C0


def uniform_operands(env, case):
    ops = env["ops"]
    seed = zlib.crc32(case.name.encode()) % (1 << 30)
    (ar, ac), (br, bc) = operand_shapes(case)
    _, A = embed(env, ar, ac, case.layout[0], FILLS["nan"])
    _, B = embed(env, br, bc, case.layout[1], FILLS["nan"])
    if A.numel():
        A.copy_(ops.uniform_pm1(seed, (ar, ac), device=env["dev"]))
        B.copy_(ops.uniform_pm1(seed + 1, (br, bc), scale=max(case.K, 1) ** -0.5, device=env["dev"]))
    C0 = ops.uniform_pm1(seed + 2, (case.M, case.N), device=env["dev"])
    return A, B, C0


def fresh_c(env, case, fill, beta, C0, rows=None):
    """The C view for one call: the whole buffer holds the fill; the view holds C0 when beta != 0 and the fill when beta == 0."""
    Cbuf, Cv = embed(env, case.M if rows is None else rows, case.N, case.layout[2], fill)
    if beta != 0:
        Cv.copy_(C0)
    return Cbuf, Cv


IDS = [c.name for c in gr.CASES]


# ------------------------------------------------------------------ 1. exact leg
@pytest.mark.parametrize("fill", sorted(FILLS))
@pytest.mark.parametrize("case", gr.CASES, ids=IDS)
def test_exact_leg(env, case, fill):
    fill = FILLS[fill]
    A, B, C0 = int_operands(env, case, fill)
    prod = product64(case, A, B)
    assert not prod.numel() or float(prod.abs().max()) < 2 ** 23       # every partial sum is exact in float32
    for alpha, beta in case.pairs:
        Cbuf, Cv = fresh_c(env, case, fill, beta, C0)
        run(env, case, A, B, Cv, alpha, beta)
        ref = alpha * prod + beta * C0.double()
        ne = Cv.double() != ref                       # a NaN differs
        if bool(ne.any()):
            rows = ne.any(1).nonzero().flatten()
            cols = ne.any(0).nonzero().flatten()
            pytest.fail(f"{case.name} alpha={alpha} beta={beta}: {int(ne.sum())} of {ne.numel()} elements differ from float64 "
                        f"({int(Cv.isnan().sum())} NaN); rows {int(rows[0])}..{int(rows[-1])}, columns {int(cols[0])}..{int(cols[-1])}; "
                        f"path {[c.kernel + ':' + c.tile for c in gr.case_path(case, beta)]}")
        Cv.fill_(fill)
        assert holds_fill(Cbuf, fill), f"{case.name} alpha={alpha} beta={beta}: the C buffer changed outside the view"


# ------------------------------------------------------------------ 2. rounding, identity and same-chain legs
def slice_starts(M):
    """Row 0, a 1000-row range across a 256-row tile seam in the middle, the tail."""
    return sorted({0, max(0, (M // 512) * 256 - 500), M - 1000})


@pytest.mark.parametrize("case", gr.CASES, ids=IDS)
def test_rounding_identity_and_chain_legs(env, case):
    torch = env["torch"]
    nan = FILLS["nan"]
    A, B, C0 = uniform_operands(env, case)
    alpha, beta = float(np.float32(0.3)), float(np.float32(case.rbeta))
    _, Cv = fresh_c(env, case, nan, beta, C0)
    got = run(env, case, A, B, Cv, alpha, beta)
    # rounding leg
    ref = alpha * product64(case, A, B) + beta * C0.double()
    absum = abs(alpha) * product64(case, A.abs(), B.abs()) + abs(beta) * C0.double().abs()
    assert_rows_close(got, lambda r0, r1: ref[r0:r1], f"{case.name} rounding leg", absum_fn=lambda r0, r1: absum[r0:r1])
    del ref, absum
    # identity leg
    _, Pv = fresh_c(env, case, nan, 0.0, C0)
    P = run(env, case, A, B, Pv, 1.0, 0.0)
    want = gr.epilogue_f32(P.cpu().numpy(), C0.cpu().numpy(), alpha, beta)
    ne = got.cpu().numpy().view(np.int32) != want.view(np.int32)
    assert not ne.any(), (f"{case.name} identity leg: {int(ne.sum())} of {ne.size} elements are not fl(fl(alpha P) + fl(beta C0)); "
                          f"path {[c.kernel + ':' + c.tile for c in gr.case_path(case, beta)]}")
    # same-chain leg
    if case.chain == "slices":
        _, Tv = fresh_c(env, case, nan, 0.0, C0)
        T = run(env, case, A, B, Tv, 2.0, 0.0)
        assert torch.equal(T, P + P), f"{case.name}: alpha = 2 is not twice alpha = 1"
        for s in slice_starts(case.M):
            _, Sv = fresh_c(env, case, nan, 0.0, C0, rows=1000)
            run(env, case, A[s:s + 1000], B, Sv, 2.0, 0.0, M=1000)
            ne = Sv != T[s:s + 1000]
            assert not bool(ne.any()), f"{case.name}: rows {s}..{s + 999} as a short product differ in {int(ne.sum())} elements"
        if case.ws == "zero":   # the optional W^T workspace: the same bits with it
            _, Wv = fresh_c(env, case, nan, 0.0, C0)
            ws = env["capi"].gemm_workspace(0, 1, case.M, case.N, case.K)
            assert ws > 0
            run(env, case, A, B, Wv, 2.0, 0.0, ws_bytes=ws)
            assert torch.equal(Wv, T), f"{case.name}: the call without the W^T workspace differs from the call with it"
    elif case.chain == "rerun":
        outs = []
        for _ in range(2):
            _, Rv = fresh_c(env, case, nan, beta, C0)
            outs.append(run(env, case, A, B, Rv, 2.0, beta))
        assert torch.equal(outs[0], outs[1]), f"{case.name}: two runs differ"
    else:
        assert case.chain is None


# ------------------------------------------------------------------ 3. an infinity inside an operand
INF_CASES = [c for c in gr.CASES if c.name.startswith("generic-")]


@pytest.mark.parametrize("case", INF_CASES, ids=[c.name for c in INF_CASES])
def test_infinity_inside_an_operand_stays_in_its_row_and_column(env, case):
    """IEEE propagation: strictly positive integer operands with +Inf at the first and last k of one row of op(A) and of one column of
    op(B) give +Inf in exactly that row and that column of C and exact integers elsewhere -- in any summation order (no Inf - Inf, no
    0 * Inf exists in the product).  The kernels' out-of-range loads are clamped INTO the matrix (to the row's first element, or to the
    last k row) and dropped later: the poisoned padding never reaches them, an infinity at those positions does -- a mask done by
    multiplication turns the row or column into NaN, a select keeps it.  Every shape here has a ragged last K-tile."""
    torch = env["torch"]
    nan, inf = FILLS["nan"], FILLS["inf"]
    gen = torch.Generator(device=env["dev"])
    gen.manual_seed(zlib.crc32(case.name.encode()))
    (ar, ac), (br, bc) = operand_shapes(case)
    _, A = embed(env, ar, ac, case.layout[0], nan)
    _, B = embed(env, br, bc, case.layout[1], nan)
    fill_small_ints(A, gen, 1, 3)
    fill_small_ints(B, gen, 1, 3)
    C0 = fill_small_ints(torch.empty((case.M, case.N), dtype=torch.float32, device=env["dev"]), gen, -3, 3)
    r0, c0 = case.M // 2, case.N // 3
    Aop, Bop = op(A, case.trans[0] == "T"), op(B, case.trans[1] == "T")      # [M, K] and [K, N] views of the same memory
    Aop[r0, 0] = Aop[r0, case.K - 1] = inf
    Bop[0, c0] = Bop[case.K - 1, c0] = inf
    prod = product64(case, A, B)
    finite = torch.ones_like(prod, dtype=torch.bool)
    finite[r0, :] = False
    finite[:, c0] = False
    assert bool((prod == inf)[~finite].all()) and bool(prod[finite].isfinite().all())
    for alpha, beta in ((1.0, 0.0), (2.0, 0.5)):
        Cbuf, Cv = fresh_c(env, case, nan, beta, C0)
        run(env, case, A, B, Cv, alpha, beta)
        ne = Cv.double() != alpha * prod + beta * C0.double()
        assert not bool(ne.any()), (f"{case.name} alpha={alpha} beta={beta}: {int(ne.sum())} elements differ, {int(Cv.isnan().sum())} are NaN "
                                    f"(row {r0} and column {c0} must be +Inf, everything else an exact integer)")
        Cv.fill_(nan)
        assert holds_fill(Cbuf, nan)


# ------------------------------------------------------------------ 4. empty products, workspace, refusals
def plain_case(trans, M, N, K, ws="full"):
    return gr.Case(f"{trans}-{M}x{N}x{K}", trans, M, N, K, "aaa", (), 0.0, ws, None)


def test_empty_outputs_return_ok_and_write_nothing(env):
    for trans in ("NN", "NT", "TN", "TT"):
        for M, N in ((0, 5), (5, 0), (0, 0)):
            case = plain_case(trans, M, N, 7)
            (ar, ac), (br, bc) = operand_shapes(case)
            _, A = embed(env, ar, ac, "a", FILLS["nan"])
            _, B = embed(env, br, bc, "a", FILLS["nan"])
            Cbuf, Cv = embed(env, M, N, "a", 7.0)
            assert status_of(env, case, A, B, Cv, 2.0, 0.5) == 0
            assert holds_fill(Cbuf, 7.0)


def test_tall_nt_without_workspace_has_the_same_bits(env):
    """The W^T workspace of the tall transB = 1 case is optional: workspace_bytes = 0 succeeds (here on gemm_kernel) and holds the
    bits of the call with the workspace (gemm_dma_kernel)."""
    torch = env["torch"]
    case = plain_case("NT", 2048 + 13, 128, 64)
    assert [c.kernel for c in gr.case_path(case, 0.0)] == ["transpose_w", "gemm_dma_kernel"]
    assert [c.kernel for c in gr.case_path(case._replace(ws="zero"), 0.0)] == ["gemm_kernel"]
    A, B, C0 = uniform_operands(env, case)
    _, C1 = fresh_c(env, case, FILLS["nan"], 0.0, C0)
    _, C2 = fresh_c(env, case, FILLS["nan"], 0.0, C0)
    run(env, case, A, B, C1, 0.3, 0.0)
    run(env, case, A, B, C2, 0.3, 0.0, ws_bytes=0)
    assert not bool(C1.isnan().any()) and torch.equal(C1, C2)


@pytest.mark.parametrize("trans,M,N,K", [("TN", 128, 128, 65536), ("TN", 128, 128, 65536 + 17), ("TN", 130, 70, 4099), ("TT", 64, 96, 200000),
                                         ("TN", 7, 2, 515)])
def test_split_k_slabs_are_required(env, trans, M, N, K):
    """transA = 1 with more than one split: one byte less than gnnx_gemm_workspace is GNNX_ERR_WORKSPACE (-4) and C is untouched --
    with or without the K % 64 remainder slab, on the LDS-DMA shape and on the generic one."""
    capi = env["capi"]
    case = plain_case(trans, M, N, K)
    need = capi.gemm_workspace(1, trans[1] == "T", M, N, K)
    assert need > 0
    A, B, C0 = int_operands(env, case, FILLS["nan"])
    Cbuf, Cv = embed(env, M, N, "a", 7.0)
    for short in (need - 1, 0):
        assert status_of(env, case, A, B, Cv, 2.0, 1.0, ws_bytes=short) == -4
        assert holds_fill(Cbuf, 7.0)
    run(env, case, A, B, Cv, 2.0, 0.0, ws_bytes=need)
    assert env["torch"].equal(Cv.double(), 2.0 * product64(case, A, B))


def test_leading_dimensions_below_the_width_are_refused(env):
    """ldc < N: GNNX_ERR_INVALID_ARG (-1); lda or ldb below the operand's row length: GNNX_ERR_SHAPE (-2), as include/gnnx.h says of
    gnnx_gemm_f32.  Nothing is launched: C keeps its contents."""
    for trans in ("NN", "NT", "TN", "TT"):
        case = plain_case(trans, 40, 24, 12)
        A, B, _ = int_operands(env, case, FILLS["nan"])
        Cbuf, Cv = embed(env, case.M, case.N, "a", 7.0)
        a_width = case.M if trans[0] == "T" else case.K
        b_width = case.K if trans[1] == "T" else case.N
        assert status_of(env, case, A, B, Cv, 1.0, 0.0, ldc=case.N - 1) == -1
        assert status_of(env, case, A, B, Cv, 1.0, 0.0, lda=a_width - 1) == -2
        assert status_of(env, case, A, B, Cv, 1.0, 0.0, ldb=b_width - 1) == -2
        assert holds_fill(Cbuf, 7.0)
