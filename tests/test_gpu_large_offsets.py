"""The tall-matrix kernels held to independent references past 2^31 element offsets (run with -m gpu on an MI355X).

A 10 M x 256 f32 matrix -- the configuration the project's metric is quoted on -- has 2.56e9 elements: element offsets pass 2^31 from
row 8 388 608 on, byte offsets pass 2^32 and 2^33.  A 32-bit row offset anywhere goes wrong here and nowhere else, so every dense
kernel that runs at this size in the step, the full layer and the training step gets, at such a shape, a comparison whose expected
value no HIP kernel of this project produced:

  * EXACT legs.  Inputs are small integers stored as f32 (entries in {-1, 0, 1}): every product is an integer and every partial sum,
    in any order, fused or split, is an integer of magnitude <= n < 2^24 -- exact in f32.  The HIP result must EQUAL the float64 result
    on EVERY element, whatever the tile geometry, split-K slabs or summation order.  This is the leg that sees a lost, duplicated or
    misplaced row anywhere in 10 M.
  * ROUNDING legs.  The bench's data (ops.uniform_pm1, W scaled by F ** -0.5): all rows against float64 on the device, sampled rows
    (helpers.sample_rows) against the CPU oracle, with the bars of tests/test_gpu_parity.py (its module docstring) -- no new number.

Every expected value is built from row chunks of at most 1 M rows (helpers.CHUNK), so no reference depends on torch's own indexing of
a tensor of more than 2^31 elements; inputs are filled chunk by chunk too.  Where a test says "same bits as ..." about two HIP results
it is an ADDED check on top of an independent one.

Leg A: the three products (X.W^T, dH.W, dH^T.X) at three row counts chosen for the tile plan of gnnx_gemm.hip launch_dma (asserted from M
       alone, so a change of the plan fails loudly), and their fused epilogues.
Leg B: the row-streaming kernels at 10 M x 256, once more on the gather pitch (320 floats: last row at element offset 3.2e9).
Leg C: 70 001-row column slices of a buffer with leading dimension 65 536 (last row at element offset 4.6e9): the CPU oracle checks
       EVERY row; plus one product on ld = 2^20 + 64, which the LDS-DMA kernel must refuse.

The condition-aware bar of node-dimension reductions, 1e-5 * max(1, |ref|, sum_k |term_k|), cannot see a lost K-tile of dH^T.X at this
size: over 10 M rows of uniform(-1, 1) data sum|term| is about 2.5e6, the bar about 25, and dropping 64 / 128 / 256 whole rows of the
reduction moves the worst of the 256 x 256 outputs by 13.8 / 18.2 / 24.3 (numpy, seed 0).  The exact leg is what sees it
(tests/test_large_offsets_cpu.py pins both facts).

Wall time on an MI355X (pytest --durations, two runs of the module on its own; most of it is 10 GB allocations, which vary from run
to run): leg A 15-21 s, leg B 16-20 s, leg C 8-12 s, the module 41-52 s; the whole GPU suite 216 s with it (202.6 s on record before).
"""
import importlib

import numpy as np
import pytest

import oracle
from tests.helpers import (assert_close, assert_no_worse_than_reference, assert_rows_close, assert_rows_equal, assert_small_equal, chunked_sum, dma_tail_round,
                           fill_small_ints, row_chunks, sample_rows, take_rows)

pytestmark = pytest.mark.gpu

HEADLINE, F = 10_000_000, 256
FIRST_ROW_PAST_2G = 2 ** 31 // F          # 8 388 608: the first row whose element offset does not fit an int
# M -> (r = whole 256-row tiles left after the rounds of one tile per CU, M % 64, the launch the last round takes)
PLAN = {10_000_000: (150, 0, "none"),                     # 39 062 tiles + 128 ragged rows on the overlapping cover tile; no tail launch
        256 * (32768 + 40) + 77: (40, 13, "128x128"),     # tail launch starts at element offset exactly 2^31; + 77 ragged rows; K % 64 slab
        256 * (32768 + 100) + 200: (100, 8, "256x128")}   # 256 x 128 tail launch from the same offset
ROW_COUNTS = sorted(PLAN, reverse=True)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


@pytest.fixture(autouse=True)
def release(env):
    """Every test starts and ends with an empty device heap (each holds up to four 10 GB matrices)."""
    yield
    env["ops"]._ws_cache.clear()
    env["torch"].cuda.empty_cache()


def host(t):
    return t.detach().cpu().numpy()


def check_plan(M):
    """The tile-plan facts the row count was chosen for, from M alone."""
    r, k64, tail = PLAN[M]
    assert dma_tail_round(M) == r and M % 64 == k64, (M, dma_tail_round(M), M % 64)
    assert tail == ("128x128" if 1 <= r <= 64 else "256x128" if 65 <= r <= 128 else "none")
    assert M // 256 > 256 and M > FIRST_ROW_PAST_2G
    if tail != "none":
        assert (M // 256 - r) * 256 * F == 2 ** 31, "the tail launch starts at element offset 2^31"
    return r


def ints(env, shape, seed, lo=-1, hi=1):
    torch = env["torch"]
    gen = torch.Generator(device=env["dev"]).manual_seed(seed)
    return fill_small_ints(torch.empty(shape, dtype=torch.float32, device=env["dev"]), gen, lo, hi)


def signed_selection(env, n, seed):
    """[n, n] with one +-1 per column (a signed permutation): A . W has entries of A, sign flipped, so column sums stay <= rows."""
    torch = env["torch"]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    W = torch.zeros((n, n), dtype=torch.float32)
    W[torch.randperm(n, generator=gen), torch.arange(n)] = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    return W.to(env["dev"])


def pitched(env, M, fill=None, seed=None):
    """(buffer [M, 320], its [:, :256] view): a matrix on the gather pitch.  fill: a sentinel value; seed: bench data in the whole buffer."""
    ops, torch = env["ops"], env["torch"]
    ld = ops.gather_row_stride(M, F)
    assert ld == 320 or M < 100_000, ld
    buf = ops.uniform_pm1(seed, (M, ld), device=env["dev"]) if seed is not None else \
        torch.full((M, ld), fill, dtype=torch.float32, device=env["dev"]) if fill is not None else torch.empty((M, ld), dtype=torch.float32, device=env["dev"])
    return buf, buf[:, :F]


def copy_rows(dst, src):
    for r0, r1 in row_chunks(src.shape[0]):
        dst[r0:r1].copy_(src[r0:r1])
    return dst


def send_list(env, M, world=8):
    """Peer-major send list of a world of 8 (ascending inside a peer): blocks at the head, across row 8 388 608, and the last 1000 rows
    (tail launch and ragged rows) go to all 7 peers; every 11th row to peer 0 as well, every 97th (+5) to peer 1; most rows to nobody."""
    torch = env["torch"]
    lo = min(FIRST_ROW_PAST_2G, M) - 600
    everyone = torch.cat([torch.arange(0, 1000), torch.arange(lo, min(lo + 1200, M)), torch.arange(M - 1000, M)]).unique()
    parts = [everyone] * (world - 1)
    parts[0] = torch.cat([everyone, torch.arange(0, M, 11)]).unique()
    parts[1] = torch.cat([everyone, torch.arange(5, M, 97)]).unique()
    idx = torch.cat(parts).to(torch.int32).to(env["dev"])
    table = env["ops"].slot_table(idx, M)
    assert table is not None
    per_row = (table >= 0).sum(1)
    for k in (0, 1, world - 1):
        assert int((per_row == k).sum()) > 0, f"no row wanted by {k} peers"
    assert int(per_row[M - 1]) == world - 1 and int(per_row[min(FIRST_ROW_PAST_2G, M - 1)]) == world - 1 and int(per_row[0]) == world - 1
    return idx, table


def assert_gathered_equal(env, got, idx, src_fn, M, what):
    """got[s] == source row idx[s] for every slot s: the source comes chunk by chunk from src_fn(r0, r1) (float64), the slots of a
    chunk are picked with torch indexing (got has far fewer than 2^31 elements)."""
    torch = env["torch"]
    idx = idx.to(torch.int64)
    assert got.shape[0] == idx.numel()
    seen = 0
    for r0, r1 in row_chunks(M):
        slots = ((idx >= r0) & (idx < r1)).nonzero().flatten()
        if slots.numel() == 0:
            continue
        want = src_fn(r0, r1)[idx[slots] - r0]
        ne = (got[slots].double() != want).any(1)
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} slots differ, first slot {int(slots[ne][0])} <- row {int(idx[slots][ne][0])}"
        seen += int(slots.numel())
    assert seen == idx.numel()


# ================================================================== leg A: the three products
@pytest.mark.parametrize("M", ROW_COUNTS)
def test_transform_product_past_2g_elements(env, M):
    """H = X . W^T (gnnx_gemm_f32, NT).  Exact leg: {-1, 0, 1} data, |H| <= 256, every element of every row equals float64.  Rounding leg:
    the bench's data, all rows against float64 and the sampled rows against oracle.linear_fwd, 1e-5 * max(1, |ref|)."""
    ops, torch = env["ops"], env["torch"]
    check_plan(M)
    X, W = ints(env, (M, F), 11), ints(env, (F, F), 12)
    Wt = W.double().t().contiguous()
    H = ops.linear_fwd(X, W)
    assert_rows_equal(H, lambda r0, r1: X[r0:r1].double() @ Wt, f"X.W^T exact, M = {M}")
    del X, H
    X = ops.uniform_pm1(1, (M, F), device=env["dev"])
    W = ops.uniform_pm1(2, (F, F), scale=F ** -0.5, device=env["dev"])
    Wt = W.double().t().contiguous()
    H = ops.linear_fwd(X, W)
    assert_rows_close(H, lambda r0, r1: X[r0:r1].double() @ Wt, f"X.W^T vs float64, M = {M}")
    rows = sample_rows(M)
    assert_close(take_rows(H, rows), oracle.linear_fwd(take_rows(X, rows), host(W)), f"X.W^T vs oracle on {rows.size} rows, M = {M}")


@pytest.mark.parametrize("M", ROW_COUNTS)
def test_input_gradient_product_past_2g_elements(env, M):
    """dX = dH . W (gnnx_gemm_f32, NN): the legs of the transform's test; the oracle is linear_bwd's dX on the sampled rows."""
    ops, torch = env["ops"], env["torch"]
    check_plan(M)
    dH, W = ints(env, (M, F), 21), ints(env, (F, F), 22)
    W64 = W.double()
    dX = ops.gemm(dH, W)
    assert_rows_equal(dX, lambda r0, r1: dH[r0:r1].double() @ W64, f"dH.W exact, M = {M}")
    del dH, dX
    dH = ops.uniform_pm1(3, (M, F), device=env["dev"])
    W = ops.uniform_pm1(2, (F, F), scale=F ** -0.5, device=env["dev"])
    W64 = W.double()
    dX = ops.gemm(dH, W)
    assert_rows_close(dX, lambda r0, r1: dH[r0:r1].double() @ W64, f"dH.W vs float64, M = {M}")
    rows = sample_rows(M)
    ref, _ = oracle.linear_bwd(take_rows(dH, rows), np.zeros((rows.size, F), dtype=np.float32), host(W), need_dw=False)
    assert_close(take_rows(dX, rows), ref, f"dH.W vs oracle on {rows.size} rows, M = {M}")


@pytest.mark.parametrize("M", ROW_COUNTS)
def test_weight_gradient_product_past_2g_elements(env, M):
    """dW = dH^T . X (gnnx_gemm_f32, TN: the reduction runs over the M rows; split-K slabs, and for M % 64 != 0 one more slab).

    Exact leg: {-1, 0, 1} data, every partial sum is an integer <= M < 2^24, so all 256 x 256 outputs equal float64 -- a lost, doubled
    or misplaced row of the reduction changes an integer.  beta = 1 on top of a {-1, 0, 1} matrix: still <= M + 1 < 2^24, exact.

    Rounding leg: the bench's data against float64 over all rows with the project's condition-aware bar 1e-5 * max(1, |ref|, sum|term|).
    That bar ALONE does not see a lost K-tile at this size: sum|term| ~ 2.5e6 gives a bar of ~25 while dropping 64 / 128 / 256 rows
    moves the worst output by 13.8 / 18.2 / 24.3 (numpy, seed 0; pinned in tests/test_large_offsets_cpu.py) -- the exact leg is what
    does.  In addition the `exact=` clause of assert_close (the GPU no further from float64 than twice the oracle's own error) against
    oracle.linear_bwd on the block rows x columns {0..15, 240..255}^2 of dW, fed those column strips of dH and X as packed M x 32
    host matrices."""
    ops, torch = env["ops"], env["torch"]
    check_plan(M)
    dH, X = ints(env, (M, F), 31), ints(env, (M, F), 32)
    ref = chunked_sum(lambda r0, r1: dH[r0:r1].double().t() @ X[r0:r1].double(), M)
    assert float(ref.abs().max()) <= M
    dW = ops.gemm(dH, X, transA=True)
    assert_small_equal(dW, ref, f"dH^T.X exact, M = {M}")
    C0 = ints(env, (F, F), 33)
    acc = C0.clone()
    ops.gemm(dH, X, transA=True, out=acc, beta=1.0)
    assert_small_equal(acc, ref + C0.double(), f"dH^T.X exact with beta = 1, M = {M}")
    del dH, X
    dH = ops.uniform_pm1(3, (M, F), device=env["dev"])
    X = ops.uniform_pm1(1, (M, F), device=env["dev"])
    ref = chunked_sum(lambda r0, r1: dH[r0:r1].double().t() @ X[r0:r1].double(), M)
    absum = chunked_sum(lambda r0, r1: dH[r0:r1].double().abs().t() @ X[r0:r1].double().abs(), M)
    dW = ops.gemm(dH, X, transA=True)
    got, ref, absum = host(dW), host(ref), host(absum)
    assert_close(got, ref, f"dH^T.X vs float64, M = {M}", absum=absum)
    sel = np.r_[0:16, 240:256]
    sel_d = torch.from_numpy(sel).to(env["dev"])
    dHs, Xs = np.empty((M, sel.size), dtype=np.float32), np.empty((M, sel.size), dtype=np.float32)
    for r0, r1 in row_chunks(M):
        dHs[r0:r1] = host(dH[r0:r1][:, sel_d])
        Xs[r0:r1] = host(X[r0:r1][:, sel_d])
    _, ref_o = oracle.linear_bwd(dHs, Xs, np.zeros((sel.size, sel.size), dtype=np.float32), need_dx=False)
    blk = np.ix_(sel, sel)
    assert_close(got[blk], ref_o, f"dH^T.X vs oracle on the corner block, M = {M}", absum=absum[blk], exact=ref[blk])


def test_input_gradient_with_relu_mask_and_column_sums_at_the_headline_size(env):
    """gnnx_gemm_relu_colsum_f32 at 10 M rows: G = (dH . W) (.) (Y > 0) and its column sums.  Exact leg: dH in {-1, 0, 1}, W a signed
    selection (one +-1 per column), so every G[i][j] = +-dH[i][k_j] is in {-1, 0, 1} and a column sum is bounded by the row count,
    1e7 < 2^24 (with a dense {-1, 0, 1} W a column sum could reach 256 * 1e7, which is NOT below 2^24); Y a seeded {0, 1} matrix."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    check_plan(M)
    dH, W, Y = ints(env, (M, F), 41), signed_selection(env, F, 42), ints(env, (M, F), 43, 0, 1)
    assert bool(((W != 0).sum(0) == 1).all()) and M < 2 ** 24
    W64 = W.double()
    ref_fn = lambda r0, r1: (dH[r0:r1].double() @ W64) * (Y[r0:r1] > 0)  # noqa: E731
    G, sums = ops.gemm_relu_colsum(dH, W, Y)
    assert_rows_equal(G, ref_fn, "(dH.W) (.) relu'(Y) exact")
    assert_small_equal(sums.reshape(1, -1), chunked_sum(lambda r0, r1: ref_fn(r0, r1).sum(0), M).reshape(1, -1), "column sums of G exact")


def test_transform_with_batchnorm_statistics_at_the_headline_size(env):
    """gnnx_gemm_bn_stats_f32 at 10 M rows on {-1, 0, 1} data: H equals the exact product; the statistics out of the epilogue against
    float64 statistics of the EXACT H with the bars of test_gpu_parity.py::test_bn_stats_from_the_transform_vs_float64 (mean within 1e-5
    of the column's standard deviation, variance within 1e-6 relative).

    The two-pass kernel (gnnx_bn_stats_f32) is NOT held to 1e-6 on this H; it is on the bench's data
    (test_batchnorm_relu_at_the_headline_size).  H here takes about a hundred distinct integer values, so the rounding error of an f32 accumulation step is the same every time
    a value recurs and the errors add up instead of averaging out: measured on an MI355X, the two-pass variance of this H is 1.1e-7 from
    float64 in the median column and 1.6e-5 in the worst, torch's own f32 sum of squares 1.3e-6 (1 M rows: 3.0e-6), while on the bench's H
    both are below 4e-7.  Its mean is within 3e-11 of the standard deviation: every row is read once."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    X, W = ints(env, (M, F), 51), ints(env, (F, F), 52)
    Wt = W.double().t().contiguous()
    ref_fn = lambda r0, r1: X[r0:r1].double() @ Wt  # noqa: E731
    H, m1, v1 = ops.linear_fwd_bn_stats(X, W)
    assert_rows_equal(H, ref_fn, "H of the statistics epilogue exact")
    m64 = chunked_sum(lambda r0, r1: ref_fn(r0, r1).sum(0), M) / M
    v64 = chunked_sum(lambda r0, r1: ((ref_fn(r0, r1) - m64) ** 2).sum(0), M) / M
    em, ev = ((m1.double() - m64).abs() / v64.sqrt()).max().item(), ((v1.double() - v64).abs() / v64).max().item()
    assert em <= 1e-5 and ev <= 1e-6, (em, ev)
    m2, _ = ops.bn_stats(H)
    assert ((m2.double() - m64).abs() / v64.sqrt()).max().item() <= 1e-5


def test_transform_with_bf16_output_at_the_headline_size(env):
    """gnnx_gemm_nt_bf16out_f32 at 10 M rows: integers up to 256 are exact in bf16 (8 significant bits), so the stored bf16 equals the
    exact product of {-1, 0, 1} data."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    X, W = ints(env, (M, F), 61), ints(env, (F, F), 62)
    Wt = W.double().t().contiguous()
    H = ops.linear_fwd_bf16(X, W)
    assert H.dtype == torch.bfloat16
    assert_rows_equal(H, lambda r0, r1: X[r0:r1].double() @ Wt, "bf16 H exact")


@pytest.mark.parametrize("M", [256 * (32768 + 40) + 77, HEADLINE])
def test_transform_with_the_pack_past_2g_elements(env, M):
    """gnnx_gemm_nt_rows_to_slots_f32, world 8: H equals the exact product, the send buffer equals H_exact[send_idx] -- rows below and above
    8 388 608, rows of the tail launch and the ragged rows, rows wanted by 0, 1 and 7 peers (send_list asserts all of that)."""
    ops, torch = env["ops"], env["torch"]
    check_plan(M)
    idx, table = send_list(env, M)
    X, W = ints(env, (M, F), 71), ints(env, (F, F), 72)
    Wt = W.double().t().contiguous()
    ref_fn = lambda r0, r1: X[r0:r1].double() @ Wt  # noqa: E731
    H = torch.full((M, F), float("nan"), dtype=torch.float32, device=env["dev"])
    send = torch.full((idx.numel(), F), float("nan"), dtype=torch.float32, device=env["dev"])
    ops.linear_fwd_rows_to_slots(X, W, H, table, send)
    assert_rows_equal(H, ref_fn, f"H of the pack epilogue exact, M = {M}")
    assert_gathered_equal(env, send, idx, ref_fn, M, f"send buffer of the pack epilogue, M = {M}")


# ================================================================== leg B: the row-streaming kernels at 10 M x 256
def test_column_sums_and_copy_at_the_headline_size(env):
    """gnnx_colsum_f32 / gnnx_colsum_copy_f32: {-1, 0, 1} data, sums (<= 1e7) equal float64; the copy on the gather pitch equals the source
    and the pad columns keep their sentinel; the sums of the pitched copy (source ld 320) are exact too."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    G = ints(env, (M, F), 81)
    ref = chunked_sum(lambda r0, r1: G[r0:r1].double().sum(0), M).reshape(1, -1)
    assert_small_equal(ops.colsum(G).reshape(1, -1), ref, "colsum exact")
    buf, copy = pitched(env, M, fill=7.0)
    sums = ops.colsum_copy(G, copy)
    assert_small_equal(sums.reshape(1, -1), ref, "colsum_copy sums exact")
    assert_rows_equal(copy, lambda r0, r1: G[r0:r1].double(), "colsum_copy copy")
    assert_rows_equal(buf[:, F:], lambda r0, r1: torch.full((r1 - r0, buf.shape[1] - F), 7.0, dtype=torch.float64, device=env["dev"]), "pad columns untouched")
    assert_small_equal(ops.colsum(copy).reshape(1, -1), ref, "colsum of a pitched source exact")
    acc0 = ints(env, (1, F), 82)                             # beta = 1 on top of {-1, 0, 1}: still <= 1e7 + 1 < 2^24
    acc = acc0.clone().reshape(-1)
    assert_small_equal(ops.colsum(copy, out=acc, beta=1.0).reshape(1, -1), ref + acc0.double(), "colsum beta = 1 exact")


def test_pack_from_the_producers_side_at_the_headline_size(env):
    """gnnx_rows_to_slots_f32 at 10 M rows, packed and pitched source: the send buffer equals X[send_idx] (torch indexing per chunk), the
    column sums riding along equal float64 ({-1, 0, 1} data)."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    idx, table = send_list(env, M)
    X = ints(env, (M, F), 91)
    ref = chunked_sum(lambda r0, r1: X[r0:r1].double().sum(0), M).reshape(1, -1)
    _, Xp = pitched(env, M)
    copy_rows(Xp, X)
    for name, src in (("packed", X), ("pitched", Xp)):
        send = torch.full((idx.numel(), F), float("nan"), dtype=torch.float32, device=env["dev"])
        sums = torch.empty(F, dtype=torch.float32, device=env["dev"])
        ops.rows_to_slots(src, table, send, colsum_out=sums)
        assert_gathered_equal(env, send, idx, lambda r0, r1: X[r0:r1].double(), M, f"rows_to_slots ({name})")
        assert_small_equal(sums.reshape(1, -1), ref, f"rows_to_slots column sums ({name})")


def test_bf16_conversion_at_the_headline_size(env):
    """gnnx_f32_to_bf16 on the bench's data, packed and with source and destination on the pitch: the bits of torch's .bfloat16() per
    chunk (both round to nearest even)."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    _, X = pitched(env, M, seed=1)
    ref_fn = lambda r0, r1: X[r0:r1].bfloat16().view(torch.int16).double()  # noqa: E731
    out = torch.empty((M, 320), dtype=torch.bfloat16, device=env["dev"])[:, :F]
    ops.to_bf16(X, out=out)
    assert_rows_equal(out.view(torch.int16), ref_fn, "to_bf16 (pitched)")
    Xc = copy_rows(torch.empty((M, F), dtype=torch.float32, device=env["dev"]), X)
    assert_rows_equal(ops.to_bf16(Xc).view(torch.int16), ref_fn, "to_bf16 (packed)")


def test_gather_and_scatter_rows_at_the_headline_size(env):
    """gnnx_gather_rows_f32 / gnnx_scatter_add_rows_f32 with indices on both sides of row 8 388 608, packed and pitched: gather equals torch
    indexing per chunk (repeated indices included); scatter-add of {-1, 0, 1} rows (sums of small integers: exact) equals index_add_
    per chunk."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    gen = torch.Generator(device="cpu").manual_seed(101)
    idx = torch.cat([torch.randint(0, M, (400_000,), generator=gen), torch.arange(FIRST_ROW_PAST_2G - 300, FIRST_ROW_PAST_2G + 300),
                     torch.arange(M - 300, M), torch.arange(0, 300), torch.randint(M - 5000, M, (20_000,), generator=gen)])
    idx = idx[torch.randperm(idx.numel(), generator=gen)].to(torch.int32).to(env["dev"])
    assert int((idx < FIRST_ROW_PAST_2G).sum()) > 1000 and int((idx >= FIRST_ROW_PAST_2G).sum()) > 1000
    X = ints(env, (M, F), 102)
    _, Xp = pitched(env, M)
    copy_rows(Xp, X)
    src_fn = lambda r0, r1: X[r0:r1].double()  # noqa: E731
    assert_gathered_equal(env, ops.gather_rows(X, idx), idx, src_fn, M, "gather_rows (packed)")
    assert_gathered_equal(env, ops.gather_rows(Xp, idx), idx, src_fn, M, "gather_rows (pitched)")
    # scatter-add: an index may repeat across calls, not within one (include/gnnx.h) -- the list made unique, applied twice
    idx = idx.unique()[torch.randperm(int(idx.unique().numel()), generator=gen).to(env["dev"])].contiguous()
    inp = ints(env, (idx.numel(), F), 103)
    idx64 = idx.to(torch.int64)

    def ref_fn(r0, r1):
        slots = ((idx64 >= r0) & (idx64 < r1)).nonzero().flatten()
        return X[r0:r1].double().index_add_(0, idx64[slots] - r0, 2 * inp[slots].double())
    Y = X.clone()
    for _ in range(2):
        ops.scatter_add_rows(inp, idx, Y)
    assert_rows_equal(Y, ref_fn, "scatter_add_rows (packed)")
    del Y
    for _ in range(2):
        ops.scatter_add_rows(inp, idx, Xp)
    assert_rows_equal(Xp, ref_fn, "scatter_add_rows (pitched)")


def test_elementwise_broadcasts_at_the_headline_size(env):
    """gnnx_rowscale_f32, gnnx_bias_add_f32, gnnx_binary_bcast_f32 (add, sub, mul, div; row and column broadcast) on the bench's data: each
    output is ONE IEEE operation, so it must equal the float64 operation rounded to f32 -- for +, -, *, / of two f32 numbers that double
    rounding is the correctly rounded f32 result (53 >= 2 * 24 + 2).  rowscale reads a pitched source, bias_add writes a pitched
    destination."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    _, Xp = pitched(env, M, seed=1)
    X = copy_rows(torch.empty((M, F), dtype=torch.float32, device=env["dev"]), Xp)
    v = ops.uniform_pm1(5, (M, 1), device=env["dev"]) + 1.5      # [0.5, 2.5): no division by zero
    b = ops.uniform_pm1(6, (1, F), device=env["dev"]) + 1.5
    rnd = lambda t: t.float().double()  # noqa: E731
    out = ops.rowscale(Xp, v.reshape(-1), out=torch.empty((M, F), dtype=torch.float32, device=env["dev"]))
    assert_rows_equal(out, lambda r0, r1: rnd(X[r0:r1].double() * v[r0:r1].double()), "rowscale (pitched source)")
    buf, outp = pitched(env, M, fill=7.0)
    ops.bias_add(X, b.reshape(-1), out=outp)
    assert_rows_equal(outp, lambda r0, r1: rnd(X[r0:r1].double() + b.double()), "bias_add (pitched destination)")
    assert_rows_equal(buf[:, F:], lambda r0, r1: torch.full((r1 - r0, buf.shape[1] - F), 7.0, dtype=torch.float64, device=env["dev"]), "bias_add pad columns")
    del buf, outp, Xp
    fns = {"add": torch.add, "sub": torch.sub, "mul": torch.mul, "div": torch.div}
    for op, fn in fns.items():
        ops.binary(op, X, v, out=out)
        assert_rows_equal(out, lambda r0, r1: rnd(fn(X[r0:r1].double(), v[r0:r1].double())), f"binary {op}, [N,F] x [N,1]")
        ops.binary(op, X, b, out=out)
        assert_rows_equal(out, lambda r0, r1: rnd(fn(X[r0:r1].double(), b.double())), f"binary {op}, [N,F] x [1,F]")
        ops.binary(op, v, X, out=out)
        assert_rows_equal(out, lambda r0, r1: rnd(fn(v[r0:r1].double(), X[r0:r1].double())), f"binary {op}, [N,1] x [N,F]")


def check_bn(env, X, dY, gamma, beta, relu, quirk, what, eps=1e-5):
    """gnnx_bn_stats_f32, gnnx_bn_relu_fwd_f32 and one backward form (textbook, or the reference-quirk form dX = g * gamma / sd) against
    float64 in chunks from the same inputs -- statistics first, then every row -- with the bars of
    test_bn_stats_from_the_transform_vs_float64 (mean within 1e-5 of the standard deviation, variance 1e-6 relative),
    test_batchnorm_relu_backward_vs_float64 (forward 1e-5 * max(1, |ref|); dbeta, dgamma 1e-5 * max(1, sum|term|); dX 1e-4 *
    max(1, max|dX|)) and, for the quirk form, of test_batchnorm_relu_backward_reference_quirk_vs_oracle (dX 1e-5 * max(1, |ref|)).

    The ReLU mask of the backward reference is the sign of the STORED forward output, which the backward kernel is handed as an input
    (it is itself held to float64 two lines earlier): a unit whose pre-activation is within rounding of 0 may fall on either side of the
    ReLU in f32, and over 2.56e9 units some do; with the mask an input, every gradient element and both sums are compared, none left out."""
    ops, torch = env["ops"], env["torch"]
    n = X.shape[0]
    mu = chunked_sum(lambda r0, r1: X[r0:r1].double().sum(0), n) / n
    v64 = chunked_sum(lambda r0, r1: ((X[r0:r1].double() - mu) ** 2).sum(0), n) / n
    rstd = 1.0 / torch.sqrt(v64 + eps)
    g64 = gamma.double() if gamma is not None else torch.ones_like(mu)
    b64 = beta.double() if beta is not None else torch.zeros_like(mu)
    xhat = lambda r0, r1: (X[r0:r1].double() - mu) * rstd  # noqa: E731
    y = lambda r0, r1: xhat(r0, r1) * g64 + b64  # noqa: E731
    mean, var = ops.bn_stats(X)
    em, ev = ((mean.double() - mu).abs() / v64.sqrt()).max().item(), ((var.double() - v64).abs() / v64).max().item()
    assert em <= 1e-5 and ev <= 1e-6, (what, em, ev)
    Y = ops.bn_relu_fwd(X, mean, var, gamma, beta, relu=relu)
    assert_rows_close(Y, lambda r0, r1: y(r0, r1).clamp_min(0) if relu else y(r0, r1), f"{what}: forward")
    g = lambda r0, r1: dY[r0:r1].double() * (Y[r0:r1] > 0) if relu else dY[r0:r1].double()  # noqa: E731
    dbeta_ref = chunked_sum(lambda r0, r1: g(r0, r1).sum(0), n)
    dgamma_ref = chunked_sum(lambda r0, r1: (g(r0, r1) * xhat(r0, r1)).sum(0), n)
    s_beta = float(chunked_sum(lambda r0, r1: g(r0, r1).abs().sum(0), n).max())
    s_gamma = float(chunked_sum(lambda r0, r1: (g(r0, r1) * xhat(r0, r1)).abs().sum(0), n).max())
    dX, dgamma, dbeta = ops.bn_relu_bwd(X, Y, dY, mean, var, gamma, relu=relu, beta=beta, reference_quirk=quirk)
    assert float((dbeta.double() - dbeta_ref).abs().max()) <= 1e-5 * max(1.0, s_beta), f"{what}: dbeta"
    assert float((dgamma.double() - dgamma_ref).abs().max()) <= 1e-5 * max(1.0, s_gamma), f"{what}: dgamma"
    if quirk:
        assert_rows_close(dX, lambda r0, r1: g(r0, r1) * g64 * rstd, f"{what}: dX (quirk)")
    else:
        dx = lambda r0, r1: g64 * rstd * (g(r0, r1) - dbeta_ref / n - xhat(r0, r1) * dgamma_ref / n)  # noqa: E731
        dx_max = max(float(dx(r0, r1).abs().max()) for r0, r1 in row_chunks(n))
        assert_rows_close(dX, dx, f"{what}: dX", rtol=1e-4, ref_scale=max(1.0, dx_max))


@pytest.mark.parametrize("relu,affine,quirk,pitch", [(True, True, False, True), (False, False, False, False), (True, True, True, False)])
def test_batchnorm_relu_at_the_headline_size(env, relu, affine, quirk, pitch):
    """BatchNorm + ReLU forward and backward at 10 M x 256 against float64 in chunks from the same inputs (statistics first, then every
    row): relu and affine on (source on the gather pitch), both off, and the reference-quirk backward."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    if pitch:
        _, X = pitched(env, M, seed=201)
    else:
        X = ops.uniform_pm1(201, (M, F), device=env["dev"])
    for r0, r1 in row_chunks(M):
        X[r0:r1].mul_(2.0).add_(0.3)
    dY = ops.uniform_pm1(204, (M, F), device=env["dev"])
    gamma = ops.uniform_pm1(202, (F,), device=env["dev"]) + 1.5 if affine else None
    beta = ops.uniform_pm1(203, (F,), scale=0.3, device=env["dev"]) if affine else None
    check_bn(env, X, dY, gamma, beta, relu, quirk, f"relu={relu} affine={affine} quirk={quirk}")


def test_batchnorm_backward_bias_gradient_exact_at_the_headline_size(env):
    """The exact leg of BatchNorm's backward column sum over 10 M rows, with the forward output NOT stored (the kernel recomputes its sign
    from X): X in {-1, +1}, so a column's mean lies strictly inside (-1, 1), the pre-activation (x - mean) / sd has the sign of x and is
    never within rounding of 0, and dbeta = sum of the {-1, 0, 1} entries of dY where x = +1 -- an integer <= 1e7 < 2^24 in any order.
    dX of the reference-quirk form, g / sd, is one IEEE division of a small integer by the f32 sd = sqrt(var + eps): compared with the
    float64 division by the kernel's own f32 var, at the quirk test's bar."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    X = ints(env, (M, F), 221, 0, 1)
    for r0, r1 in row_chunks(M):
        X[r0:r1].mul_(2.0).sub_(1.0)
    dY = ints(env, (M, F), 222)
    mean, var = ops.bn_stats(X)
    assert float(mean.abs().max()) < 0.5
    ref = chunked_sum(lambda r0, r1: (dY[r0:r1].double() * (X[r0:r1] > 0)).sum(0), M).reshape(1, -1)
    for quirk in (False, True):
        dX, dgamma, dbeta = ops.bn_relu_bwd(X, None, dY, mean, var, None, relu=True, reference_quirk=quirk)
        assert_small_equal(dbeta.reshape(1, -1), ref, f"dbeta exact (quirk={quirk})")
    sd = torch.sqrt(var.double() + 1e-5)
    assert_rows_close(dX, lambda r0, r1: dY[r0:r1].double() * (X[r0:r1] > 0) / sd, "dX (quirk) of integer data")


def test_relu_mask_backward_without_batchnorm_at_the_headline_size(env):
    """gnnx_bn_relu_bwd_f32 without statistics is the ReLU mask alone: dX equals dY where the stored forward output is positive, else 0 --
    no rounding, so every element is equal; and the forward is max(x, 0)."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    X = ops.uniform_pm1(211, (M, F), device=env["dev"])
    dY = ops.uniform_pm1(212, (M, F), device=env["dev"])
    Y = ops.bn_relu_fwd(X, relu=True)
    assert_rows_equal(Y, lambda r0, r1: X[r0:r1].double().clamp_min(0), "relu forward")
    dX, _, _ = ops.bn_relu_bwd(X, Y, dY, relu=True)
    assert_rows_equal(dX, lambda r0, r1: dY[r0:r1].double() * (X[r0:r1] > 0), "relu mask backward")


def first_argmax(torch, x):
    """The FIRST index of each row's maximum (reference functional.h:59-61), whatever torch.argmax does with ties."""
    c = x.shape[1]
    cols = torch.arange(c, device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, cols, torch.full_like(cols, c)).min(1).values


def check_softmax(env, logits, n, grad_view=None):
    """gnnx_softmax_ce_f32 (+ fused bias gradient), gnnx_softmax_ce_rows_f32, gnnx_argmax_rows_f32, gnnx_accuracy_rows_f32 against a float64
    log-softmax per chunk, with the bars of test_softmax_cross_entropy_shapes_and_fused_bias_gradient: loss 1e-5 * max(1, |ref|), gradient
    rows 1e-4 / n absolute, bias gradient 1e-5 * max_c sum_i |p_ic|."""
    ops, torch = env["ops"], env["torch"]
    c = logits.shape[1]
    target = ((7 * torch.arange(n, device=env["dev"]) + 3) % c).to(torch.int32)

    def logp(r0, r1):
        x = logits[r0:r1].double()
        return x - torch.logsumexp(x, 1, keepdim=True)

    def grad(r0, r1, div):
        p = logp(r0, r1).exp()
        p[torch.arange(r1 - r0, device=p.device), target[r0:r1].long()] -= 1.0
        return p / div

    nll = lambda r0, r1: -logp(r0, r1).gather(1, target[r0:r1].long().reshape(-1, 1)).reshape(-1)  # noqa: E731
    loss_ref = float(chunked_sum(lambda r0, r1: nll(r0, r1).sum(), n)) / n
    db = torch.full((c,), 7.0, dtype=torch.float32, device=env["dev"])
    loss, d = ops.softmax_ce(logits, target, colsum_out=db, grad_out=grad_view)
    assert abs(float(loss) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref)), (float(loss), loss_ref)
    assert_rows_close(d, lambda r0, r1: grad(r0, r1, n), "softmax_ce gradient", atol=1e-5 / n * 10)
    db_ref = chunked_sum(lambda r0, r1: grad(r0, r1, n).sum(0), n)
    db_abs = float(chunked_sum(lambda r0, r1: grad(r0, r1, n).abs().sum(0), n).max())
    assert float((db.double() - db_ref).abs().max()) <= 1e-5 * max(db_abs, 1e-12)
    # a 1 % row list spread over all rows (+ the rows across 2^31 elements and the last rows)
    rows = torch.cat([torch.arange(37, n, 100), torch.arange(max(0, min(FIRST_ROW_PAST_2G, n) - 50), min(FIRST_ROW_PAST_2G + 50, n)),
                      torch.arange(n - 20, n)]).unique().to(torch.int32).to(env["dev"])
    nl = int(rows.numel())
    listed = torch.zeros(n, dtype=torch.bool, device=env["dev"])
    listed[rows.long()] = True
    loss_rows_ref = float(chunked_sum(lambda r0, r1: (nll(r0, r1) * listed[r0:r1]).sum(), n)) / nl
    d.zero_()
    db.fill_(7.0)
    loss_r, d_r = ops.softmax_ce_rows(logits, target, rows, colsum_out=db, grad_out=d)
    assert abs(float(loss_r) - loss_rows_ref) <= 1e-5 * max(1.0, abs(loss_rows_ref)), (float(loss_r), loss_rows_ref)
    rows_grad = lambda r0, r1: grad(r0, r1, nl) * listed[r0:r1].reshape(-1, 1)  # noqa: E731
    assert_rows_close(d_r, rows_grad, "softmax_ce_rows gradient (unlisted rows stay zero)", atol=1e-5 / nl * 10)
    db_ref = chunked_sum(lambda r0, r1: rows_grad(r0, r1).sum(0), n)
    db_abs = float(chunked_sum(lambda r0, r1: rows_grad(r0, r1).abs().sum(0), n).max())
    assert float((db.double() - db_ref).abs().max()) <= 1e-5 * max(db_abs, 1e-12)
    pred = ops.argmax_rows(logits)
    assert_rows_equal(pred.reshape(-1, 1), lambda r0, r1: first_argmax(torch, logits[r0:r1]).double().reshape(-1, 1), "argmax_rows")
    hit = lambda r0, r1: first_argmax(torch, logits[r0:r1]) == target[r0:r1]  # noqa: E731
    assert ops.accuracy(logits, target) == (int(chunked_sum(lambda r0, r1: hit(r0, r1).sum(), n)), n)
    assert ops.accuracy(logits, target, rows) == (int(chunked_sum(lambda r0, r1: (hit(r0, r1) & listed[r0:r1]).sum(), n)), nl)


def test_softmax_cross_entropy_at_the_headline_size(env):
    """The loss kernels with n = 10 M rows, c = 256 classes, the gradient written on the gather pitch (GcnStack.grad_buffer)."""
    ops, torch = env["ops"], env["torch"]
    M = HEADLINE
    logits = ops.uniform_pm1(301, (M, F), device=env["dev"])
    for r0, r1 in row_chunks(M):
        logits[r0:r1].mul_(3.0)
    _, G = pitched(env, M)
    check_softmax(env, logits, M, grad_view=G)


# ================================================================== leg C: wide pitch, 70 001 rows, every row on the CPU oracle
WIDE_LD, WIDE_ROWS, WIDE_COL0 = 65_536, 70_001, 1024
assert (WIDE_ROWS - 1) * WIDE_LD > 2 ** 32


def wide(env, t=None, n=WIDE_ROWS, f=F, ld=WIDE_LD, dtype=None, fill=None):
    """A [n, f] column slice of an uninitialised [n, ld] buffer (only the slice is touched); filled through the slice from t."""
    torch = env["torch"]
    buf = torch.empty((n, ld), dtype=dtype or (t.dtype if t is not None else torch.float32), device=env["dev"])
    v = buf[:, WIDE_COL0:WIDE_COL0 + f]
    assert v.stride(0) == ld
    if t is not None:
        v.copy_(t)
    elif fill is not None:
        v.fill_(fill)
    return v


def test_products_on_a_wide_pitch_vs_oracle_every_row(env):
    """The three products and their epilogues with every operand a 70 001-row column slice of an ld = 65 536 buffer (last row at element
    offset 4.6e9): the bits of the packed call (added check), and the packed result against the oracle on ALL rows -- products 1e-5 *
    max(1, |ref|), dW with the condition-aware bar and the float64 clause, which at 70 k rows is sharp."""
    ops, torch = env["ops"], env["torch"]
    n = WIDE_ROWS
    X = ops.uniform_pm1(1, (n, F), device=env["dev"])
    dH = ops.uniform_pm1(3, (n, F), device=env["dev"])
    W = ops.uniform_pm1(2, (F, F), scale=F ** -0.5, device=env["dev"])
    Xw, dHw = wide(env, X), wide(env, dH)
    Xh, dHh, Wh = host(X), host(dH), host(W)
    H = ops.linear_fwd(X, W)
    assert torch.equal(ops.linear_fwd(Xw, W, out=wide(env)), H)
    assert_close(host(H), oracle.linear_fwd(Xh, Wh), "X.W^T (all rows)")
    dX = ops.gemm(dH, W)
    assert torch.equal(ops.gemm(dHw, W, out=wide(env)), dX)
    rdX, rdW = oracle.linear_bwd(dHh, Xh, Wh)
    assert_close(host(dX), rdX, "dH.W (all rows)")
    dW = ops.gemm(dH, X, transA=True)
    assert torch.equal(ops.gemm(dHw, Xw, transA=True), dW)
    d64, x64 = dHh.astype(np.float64), Xh.astype(np.float64)
    assert_close(host(dW), rdW, "dH^T.X", absum=np.abs(d64).T @ np.abs(x64), exact=d64.T @ x64)
    # fused epilogues: wide == packed (same bits), packed against float64 / exact references
    Y = ops.uniform_pm1(4, (n, F), device=env["dev"])
    G, sums = ops.gemm_relu_colsum(dH, W, Y)
    Gw, sums_w = ops.gemm_relu_colsum(dHw, W, wide(env, Y), out=wide(env))
    assert torch.equal(Gw, G) and torch.equal(sums_w, sums)
    g64 = (d64 @ Wh.astype(np.float64)) * (host(Y) > 0)
    assert_close(host(G), (rdX * (host(Y) > 0)).astype(np.float32), "(dH.W) (.) relu'(Y)")
    assert_close(host(sums), g64.sum(0), "column sums of G", absum=np.abs(g64).sum(0))
    Hs, m1, v1 = ops.linear_fwd_bn_stats(X, W)
    Hs_w, m1w, v1w = ops.linear_fwd_bn_stats(Xw, W, out=wide(env))
    assert torch.equal(Hs_w, Hs) and torch.equal(m1w, m1) and torch.equal(v1w, v1) and torch.equal(Hs, H)
    h64 = x64 @ Wh.astype(np.float64).T
    assert (np.abs(host(m1) - h64.mean(0)) / h64.std(0)).max() <= 1e-5 and (np.abs(host(v1) - h64.var(0)) / h64.var(0)).max() <= 1e-6
    Hb = ops.linear_fwd_bf16(X, W)
    assert torch.equal(ops.linear_fwd_bf16(Xw, W, out=wide(env, dtype=torch.bfloat16)), Hb)
    assert torch.equal(Hb, torch.from_numpy(host(H)).bfloat16().to(env["dev"])), "bf16 H = the oracle-checked H rounded to nearest even"
    idx, table = send_list(env, n)
    want = torch.from_numpy(host(H)[host(idx)]).to(env["dev"])
    Hp, send = wide(env, fill=float("nan")), wide(env, n=idx.numel(), fill=float("nan"))
    ops.linear_fwd_rows_to_slots(Xw, W, Hp, table, send)
    assert torch.equal(Hp, H) and torch.equal(send, want)


def test_lds_dma_product_refuses_a_pitch_its_offsets_cannot_hold(env):
    """ld = 2^20 + 64, 3000 rows: 256 rows x ld >= 2^28 elements, the per-lane 32-bit byte offsets of the LDS-DMA kernel cannot hold a tile,
    launch_dma_geo must refuse and the generic kernel take over -- with the oracle's values (element offsets pass 2^31 again)."""
    ops, torch = env["ops"], env["torch"]
    n, ld = 3000, 2 ** 20 + 64
    assert 256 * ld >= 2 ** 28 > 256 * WIDE_LD and (n - 1) * ld > 2 ** 31
    X = ops.uniform_pm1(1, (n, F), device=env["dev"])
    W = ops.uniform_pm1(2, (F, F), scale=F ** -0.5, device=env["dev"])
    Xw = wide(env, X, n=n, ld=ld)
    Hw = wide(env, n=n, ld=ld, fill=float("nan"))
    ops.linear_fwd(Xw, W, out=Hw)
    ref = oracle.linear_fwd(host(X), host(W))
    assert_close(host(Hw), ref, "X.W^T on ld = 2^20 + 64 (all rows)")
    assert_close(host(ops.linear_fwd(X, W)), ref, "X.W^T packed")
    dXw = wide(env, n=n, ld=ld, fill=float("nan"))
    ops.gemm(Xw, W, out=dXw)
    rdX, _ = oracle.linear_bwd(host(X), np.zeros((n, F), dtype=np.float32), host(W), need_dw=False)
    assert_close(host(dXw), rdX, "dH.W on ld = 2^20 + 64 (all rows)")


def test_row_streaming_kernels_on_a_wide_pitch(env):
    """Leg B's entry points that take leading dimensions, on 70 001-row slices of ld = 65 536 buffers: the bits of the packed call (added
    check) and the packed result against torch / float64 / the oracle on every row."""
    ops, torch = env["ops"], env["torch"]
    n = WIDE_ROWS
    X = ops.uniform_pm1(1, (n, F), device=env["dev"])
    Xw, Xh = wide(env, X), host(X)
    x64 = Xh.astype(np.float64)
    s = ops.colsum(X)
    assert torch.equal(ops.colsum(Xw), s)
    assert_close(host(s), oracle.colsum(Xh), "colsum", absum=np.abs(x64).sum(0), exact=x64.sum(0))
    cp = wide(env, fill=7.0)
    assert torch.equal(ops.colsum_copy(Xw, cp), s) and torch.equal(cp, X)
    idx, table = send_list(env, n)
    want = X[idx.long()]
    send = wide(env, n=idx.numel(), fill=float("nan"))
    sums = torch.empty(F, dtype=torch.float32, device=env["dev"])
    ops.rows_to_slots(Xw, table, send, colsum_out=sums)
    assert torch.equal(send, want) and torch.equal(sums, s)
    assert torch.equal(ops.gather_rows(Xw, idx, out=wide(env, n=idx.numel())), want)
    assert torch.equal(ops.to_bf16(Xw, out=wide(env, dtype=torch.bfloat16)), X.bfloat16())
    uniq = idx.unique().flip(0).contiguous()                 # no index twice within one scatter call (include/gnnx.h)
    Yi, inp = ints(env, (n, F), 401), ints(env, (uniq.numel(), F), 402)
    Yw = wide(env, Yi)
    ops.scatter_add_rows(wide(env, inp, n=uniq.numel()), uniq, Yw)
    assert torch.equal(Yw, Yi.double().index_add_(0, uniq.long(), inp.double()).float())
    v = ops.uniform_pm1(5, (n, 1), device=env["dev"]) + 1.5
    b = ops.uniform_pm1(6, (1, F), device=env["dev"]) + 1.5
    assert torch.equal(ops.rowscale(Xw, v.reshape(-1), out=wide(env)), (X.double() * v.double()).float())
    assert torch.equal(ops.bias_add(Xw, b.reshape(-1), out=wide(env)), (X.double() + b.double()).float())
    for op, fn in {"add": torch.add, "sub": torch.sub, "mul": torch.mul, "div": torch.div}.items():
        assert torch.equal(ops.binary(op, X, v, out=wide(env)), fn(X.double(), v.double()).float()), op
        assert torch.equal(ops.binary(op, X, b, out=wide(env)), fn(X.double(), b.double()).float()), op


def test_batchnorm_and_loss_on_a_wide_pitch_vs_oracle_every_row(env):
    """BatchNorm + ReLU (forward, textbook and reference-quirk backward) and the loss kernels on 70 001-row slices of ld = 65 536 buffers.
    The oracle's BatchNorm takes its statistics over the whole matrix, so this is where it checks every row: oracle.bn_relu_fwd and
    oracle.bn_relu_bwd_quirk with the bars of test_golden_full_layer_with_batchnorm_relu and
    test_batchnorm_relu_backward_reference_quirk_vs_oracle; the float64 legs are leg B's (check_bn, check_softmax), run on the wide
    operands."""
    ops, torch = env["ops"], env["torch"]
    n = WIDE_ROWS
    X = ops.uniform_pm1(201, (n, F), device=env["dev"]) * 2.0 + 0.3
    dY = ops.uniform_pm1(204, (n, F), device=env["dev"])
    gamma = ops.uniform_pm1(202, (F,), device=env["dev"]) + 1.5
    beta = ops.uniform_pm1(203, (F,), scale=0.3, device=env["dev"])
    Xw, dYw = wide(env, X), wide(env, dY)
    check_bn(env, Xw, dYw, gamma, beta, True, False, "wide, textbook")
    check_bn(env, Xw, dYw, gamma, beta, True, True, "wide, quirk")
    check_bn(env, Xw, dYw, None, None, False, False, "wide, no relu, no affine")
    mean, var = ops.bn_stats(Xw)
    mp, vp = ops.bn_stats(X)
    assert torch.equal(mean, mp) and torch.equal(var, vp)
    Xh, dYh, gh, bh = host(X), host(dY), host(gamma), host(beta)
    x64 = Xh.astype(np.float64)
    rY, rmean, rvar = oracle.bn_relu_fwd(Xh, gh, bh)
    # the oracle's statistics are the reference's sequential f32 sums: over 70 001 rows its variance is itself 1.7e-5 from float64
    # (measured), so two correct sums cannot agree to 1e-5 -- the project's rule for node-dimension reductions applies: the GPU no
    # further from float64 than the oracle is.  The row-streaming passes are then fed the ORACLE'S statistics and held to its rows.
    assert_no_worse_than_reference(host(mean), rmean, x64.mean(0), "batch mean vs oracle")
    assert_no_worse_than_reference(host(var), rvar, x64.var(0), "batch var vs oracle")
    rm, rv = torch.from_numpy(rmean).to(env["dev"]), torch.from_numpy(rvar).to(env["dev"])
    Y = ops.bn_relu_fwd(Xw, rm, rv, gamma, beta, relu=True, out=wide(env))
    assert torch.equal(Y, ops.bn_relu_fwd(X, rm, rv, gamma, beta, relu=True))
    assert_close(host(Y), rY, "BatchNorm + ReLU vs oracle (all rows)")
    sd_ok = np.power(rvar + np.float32(1e-5), np.float32(0.5), dtype=np.float32) == np.sqrt(rvar + np.float32(1e-5), dtype=np.float32)
    assert sd_ok.any() and np.array_equal(host(Y)[:, sd_ok], rY[:, sd_ok]), "bit-exact where powf(v, 0.5) == sqrtf(v), as in the golden test"
    dX, dgamma, dbeta = ops.bn_relu_bwd(Xw, None, dYw, rm, rv, gamma, relu=True, beta=beta, reference_quirk=True)
    dXp, dgp, dbp = ops.bn_relu_bwd(X, None, dY, rm, rv, gamma, relu=True, beta=beta, reference_quirk=True)
    assert torch.equal(dX, dXp) and torch.equal(dgamma, dgp) and torch.equal(dbeta, dbp)
    rX, rgamma, rbeta = oracle.bn_relu_bwd_quirk(Xh, dYh, gh, bh)
    Y64 = ((x64 - x64.mean(0)) / np.sqrt(x64.var(0) + 1e-5)) * gh + bh
    safe = np.abs(Y64) > 1e-4
    err = np.abs(host(dX) - rX) / np.maximum(1.0, np.abs(rX))
    assert err[safe].max() <= 1e-5
    # the sums: the quirk test compares them only when no unit is within 1e-4 of the ReLU's edge; over 18 M units some are, and each may
    # fall on either side in the oracle's f32 and in the kernel's, moving a column's sum by its own term: that much is added per column
    g = np.abs(dYh.astype(np.float64))
    t_gamma = g * np.abs(Y64 - bh) / np.abs(gh)
    assert (np.abs(host(dbeta) - rbeta) <= 1e-5 * max(1.0, g.sum(0).max()) + (g * ~safe).sum(0)).all()
    assert (np.abs(host(dgamma) - rgamma) <= 1e-5 * max(1.0, t_gamma.sum(0).max()) + (t_gamma * ~safe).sum(0)).all()
    # the loss kernels: logits and the gradient buffer on the wide pitch; the oracle's loss on all rows
    logits = ops.uniform_pm1(301, (n, F), device=env["dev"]) * 3.0
    Lw = wide(env, logits)
    check_softmax(env, Lw, n, grad_view=wide(env))
    target = ((7 * np.arange(n) + 3) % F).astype(np.int32)
    loss, _ = ops.softmax_ce(Lw, torch.from_numpy(target).to(env["dev"]), want_grad=False)
    ref = oracle.cross_entropy(host(logits), target)
    assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref))
