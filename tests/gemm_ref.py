"""The contract of gnnx_gemm_f32 (include/gnnx.h) restated for its tests: which kernels serve a call (gemm_path), the one arithmetic
every epilogue must share (epilogue_f32), and the shape table (CASES) that tests/test_gemm_contract_cpu.py proves to reach every
dispatch cell and tests/test_gpu_gemm_contract.py runs on the GPU.

gemm_path restates the host-side dispatch of csrc/gnnx_gemm.hip -- pick_tile, choose_splits, dma_shape_ok, dma_tn_shape_ok,
launch_dma's tile plan, launch_stream's conditions and the order in which gnnx_gemm_f32 tries them -- as spmm_ref.spmm_cell does for
the aggregation: it proves coverage of the table and is never a second implementation of the arithmetic.  Nothing here restates a
summation order: every exact comparison of the GPU file is independent of the order in which a kernel adds its products.

Assumptions of gemm_path (they hold for every case of the table): the workspace is 16-byte aligned, and every leading dimension is
far below the 2^28-byte per-lane offset limits of the LDS-DMA and streaming kernels."""
import collections

import numpy as np

NUM_CU = 256                                                             # gnnx_common.h kNumCU
CFG = {"kSquare": (128, 128, 32), "kWide": (128, 256, 16), "kTall32": (256, 256, 32)}   # BM, BN, BK of CfgDefault / CfgWide / CfgTall32
MIN_KSTEPS_PER_SPLIT = 8                                                 # choose_splits: "keep >= 8 K-steps per split"
MAX_SPLITS = 1024

# kernel: "gemm_kernel" | "gemm_stream_kernel" | "gemm_dma_kernel" | "gemm_dma_tn_kernel" | "splitk_reduce_kernel" | "transpose_w" |
#         "refused" (GNNX_ERR_WORKSPACE).  layout: the (a_kc, b_kc) template pair as "NN" / "NT" / "TN" / "TT" (transA, transB), the
# layout of B alone for the streaming kernel, "" where a kernel has one layout.  tile: a CFG name for the register-staged kernels,
# "256x256" / "256x128" / "256x128:NG" (guarded last column tile) / "128x128" for the LDS-DMA ones.  rows: rows of C the launch writes
# (a split-K launch writes slabs: rows of the product it covers).  splits: gridDim.z; for the reduction the number of slabs it adds.
Cell = collections.namedtuple("Cell", "kernel layout tile vec_a vec_b rows splits")


def ceil_div(a, b):
    return -(-a // b)


def pick_tile(M, N):
    if N <= 128:
        return "kSquare"
    return "kTall32" if M >= 256 else "kWide"


def choose_splits(M, N, K):
    bm, bn, bk = CFG[pick_tile(M, N)]
    tiles = ceil_div(M, bm) * ceil_div(N, bn)
    ksteps = ceil_div(K, bk)
    per_cu = 1 if bm * bn >= 256 * 256 else 2
    want = min(ceil_div(per_cu * NUM_CU, tiles), ksteps // MIN_KSTEPS_PER_SPLIT)
    return max(1, min(want, MAX_SPLITS))


def dma_shape_ok(M, N, K):
    return K % 64 == 0 and N % 4 == 0 and N >= 64 and M >= 8 * 256


def dma_tn_shape_ok(M, N, K):
    return M % 128 == 0 and N % 128 == 0 and K % 64 == 0 and K >= 64 * 1024


def gemm_workspace(transA, transB, M, N, K):
    """gnnx_gemm_workspace: bytes."""
    if transA and M > 0 and N > 0 and K > 0:
        splits = choose_splits(M, N, K)
        return 4 * (splits + 1) * M * N if splits > 1 else 0
    if not transA and transB and dma_shape_ok(M, N, K):
        return 4 * K * N
    return 0


def _dma_plan(M, N):
    """launch_dma<Epi::kPlain> on aligned operands of an eligible shape: [(tile, rows)] -- whole rounds on the main geometry and the last
    partly filled round on smaller tiles (launch_dma_with_tail), else one launch whose last tile overlaps its neighbour."""
    geo_rows = {"256x256": 256, "256x128": 256, "256x128:NG": 256, "128x128": 128}
    mt256 = M // 256
    r = mt256 % NUM_CU
    if mt256 > NUM_CU and r > 0:
        tail = None
        if N == 256 and r <= NUM_CU // 4:
            tail = ("256x256", "128x128")
        elif N == 256 and r <= NUM_CU // 2:
            tail = ("256x256", "256x128")
        elif N == 128 and r <= NUM_CU // 2:
            tail = ("256x128", "128x128")
        if tail:
            rows_main = (mt256 - r) * 256
            rest = M - rows_main
            return [(tail[0], rows_main)] + ([(tail[1], rest)] if rest >= geo_rows[tail[1]] else [])
    tile = "256x256" if N % 256 == 0 else "256x128" if N % 128 == 0 else "256x128:NG"
    return [(tile, M)] if M >= geo_rows[tile] else []


def _stream_rows(M, N, K, b_kc):
    """launch_stream: (tile, rows) of the leading rows the streaming kernel takes, or None."""
    tile = pick_tile(M, N)
    if tile == "kWide" or (b_kc and tile == "kTall32"):
        return None
    bm, bn, bk = CFG[tile]
    if K % bk or N % bn:
        return None
    m_tiles, cols = M // bm, N // bn
    if m_tiles * cols < 4 * NUM_CU * (1 if tile == "kTall32" else 2):
        return None
    return tile, m_tiles * bm


def gemm_path(transA, transB, M, N, K, beta, aligned_a, aligned_b, aligned_c, workspace_bytes):
    """The ordered launches that serve gnnx_gemm_f32(transA, transB, M, N, K, ..., beta, ...) as a list of Cell.  aligned_x: the
    operand's pointer is 16-byte aligned AND its leading dimension is a multiple of 4 (the two conditions the kernels always ask
    for together).  workspace_bytes: what the caller passes."""
    if M == 0 or N == 0:
        return []
    trans = ("T" if transA else "N") + ("T" if transB else "N")
    a_kc, b_kc = not transA, bool(transB)
    va = bool(aligned_a and (K % 4 == 0 if a_kc else M % 4 == 0))
    vb = bool(aligned_b and (K % 4 == 0 if b_kc else N % 4 == 0))
    splits = choose_splits(M, N, K) if transA and K > 0 else 1
    k_dma = K - K % 64 if transA and not transB and splits > 1 and dma_tn_shape_ok(M, N, K - K % 64) else 0
    if splits > 1 and workspace_bytes < gemm_workspace(transA, transB, M, N, K):
        return [Cell("refused", trans, "", va, vb, 0, splits)]
    cells, rows_left = [], M
    if a_kc and splits == 1 and beta == 0 and K > 0 and dma_shape_ok(M, N, K) and (not b_kc or workspace_bytes >= 4 * K * N):
        if b_kc:
            cells.append(Cell("transpose_w", "", "", False, False, 0, 1))
        if aligned_a and (b_kc or aligned_b) and aligned_c:      # W^T in the workspace is aligned and N % 4 == 0
            for tile, rows in _dma_plan(M, N):
                cells.append(Cell("gemm_dma_kernel", "", tile, True, True, rows, 1))
                rows_left -= rows
        if rows_left == 0:
            return cells
    if a_kc and splits == 1 and beta == 0 and va and vb and K > 0:
        took = _stream_rows(rows_left, N, K, b_kc)
        if took:
            cells.append(Cell("gemm_stream_kernel", "T" if b_kc else "N", took[0], True, True, took[1], 1))
            rows_left -= took[1]
            if rows_left == 0:
                return cells
    tile = pick_tile(rows_left, N)
    reduce_slabs = splits
    if k_dma > 0 and aligned_a and aligned_b:
        cells.append(Cell("gemm_dma_tn_kernel", "", "256x256" if M % 256 == 0 and N % 256 == 0 else "128x128", True, True, M, splits))
        if k_dma < K:                                            # the last K % 64 rows: one more slab
            cells.append(Cell("gemm_kernel", trans, tile, va, vb, M, 1))
            reduce_slabs = splits + 1
    else:                                                        # k_dma > 0 here: the LDS-DMA kernel declined (alignment)
        cells.append(Cell("gemm_kernel", trans, tile, va, vb, rows_left, splits))
    if splits > 1:
        cells.append(Cell("splitk_reduce_kernel", "", "", False, False, M, reduce_slabs))
    return cells


def epilogue_f32(P, C0, alpha, beta):
    """fl(fl(alpha * P) + fl(beta * C0)) in float32, three roundings; beta == 0: fl(alpha * P), and C0 is not read.  The arithmetic of
    `v = alpha * acc; if (beta != 0) v += beta * C` compiled without contraction (csrc/Makefile: -ffp-contract=off)."""
    P = np.asarray(P, dtype=np.float32)
    v = np.float32(alpha) * P
    if np.float32(beta) != 0:
        v = v + np.float32(beta) * np.asarray(C0, dtype=np.float32)
    assert v.dtype == np.float32
    return v


# ------------------------------------------------------------------------------------------------ the shape table
# layout: one letter per operand (A, B, C).  "a": a view at a 16-byte aligned offset of a buffer whose pitch is a multiple of 4 (the
# VEC flags then depend on the shape alone); "o": a view at column offset 1 of a buffer with an odd pitch (no vector access is legal).
# Either way the view lies inside a larger buffer: rows before and after, columns left and right, pitch wider than the width.
# pairs: the (alpha, beta) of the exact leg.  rbeta: beta of the rounding and identity legs (alpha = 0.3).  ws: "full" = what
# gnnx_gemm_workspace asks for, "zero" = none.  chain: "slices" = 1000-row slices recomputed as short products equal the tall result,
# "rerun" = two runs give the same bits (split-K has no short form), None = one generic launch.
Case = collections.namedtuple("Case", "name trans M N K layout pairs rbeta ws chain")

P3 = ((2.0, 0.0), (1.0, 0.5), (-0.5, -1.0))       # every alpha and three of the four betas; beta = 1 is in the GAT and TN cases
RBETA = -1.7


def _case(name, trans, M, N, K, layout="aaa", pairs=P3, rbeta=RBETA, ws="full", chain=None):
    return Case(f"{name}-{trans}-{M}x{N}x{K}-{layout}", trans, M, N, K, layout, tuple(pairs), rbeta, ws, chain)


def _build_cases():
    out = []
    all_trans = ("NN", "NT", "TN", "TT")
    # generic kernel: the issue's six shapes, packed (the shape decides the VEC flags) and with every operand off the 16-byte grid
    for shape in ((1, 1, 1), (130, 130, 130), (513, 257, 33), (200, 257, 40), (300, 130, 700), (64, 64, 31)):
        for trans in all_trans:
            chain = "rerun" if trans[0] == "T" and shape == (300, 130, 700) else None
            out.append(_case("generic", trans, *shape, chain=chain))
            out.append(_case("generic", trans, *shape, layout="ooo", pairs=((-0.5, 0.5),), chain=chain))
    # the six shapes leave VEC cells empty (NT and TN make both flags from one dimension): one shape per tile with every dimension a
    # multiple of 4 and a whole first tile (the unguarded store), each operand in turn off the grid
    for shape in ((132, 128, 36), (132, 260, 20), (260, 260, 36)):
        for trans in all_trans:
            out.append(_case("vec", trans, *shape, pairs=((2.0, 0.0), (-0.5, 1.0))))
            out.append(_case("vec", trans, *shape, layout="oaa", pairs=((2.0, 0.0),)))
            out.append(_case("vec", trans, *shape, layout="aoa", pairs=((2.0, 0.0),)))
    # GAT's skinny products (ops.gat_* : ER = H.A^T, dH += dER.A, dA = dER^T.H) and one-row / one-column outputs
    out.append(_case("gat_er", "NT", 40001, 2, 128))
    out.append(_case("gat_dh", "NN", 40001, 128, 2, pairs=((1.0, 1.0), (2.0, 1.0), (-0.5, 0.5))))
    out.append(_case("gat_da", "TN", 2, 128, 40001, chain="rerun"))
    out.append(_case("skinny", "TN", 7, 2, 515, chain="rerun"))
    for trans in all_trans:
        out.append(_case("row", trans, 1, 257, 70, pairs=((2.0, -1.0),)))
        out.append(_case("col", trans, 300, 1, 70, pairs=((-0.5, 0.5),)))
    # K = 0: C = beta * C (no load is issued: the first loads of gemm_kernel sit behind kbeg < kend)
    for trans, shape in (("NN", (130, 70, 0)), ("TN", (130, 70, 0)), ("NN", (256, 128, 0))):
        out.append(_case("k0", trans, *shape, pairs=((2.0, 0.0), (2.0, 0.5))))
    # generic split-K: >= 256 splits, a few, 2 (generic-TN-300x130x700 and skinny above)
    out.append(_case("splitk", "TN", 64, 96, 200000, chain="rerun"))
    out.append(_case("splitk", "TT", 64, 96, 200000, chain="rerun"))
    out.append(_case("splitk", "TN", 130, 70, 4099, pairs=((2.0, -1.0), (1.0, 0.5), (-0.5, 0.0)), chain="rerun"))
    # streaming kernel (beta = 0 paths): kSquare on both B layouts, kTall32, and the tall X.W^T called without the W^T workspace
    b0 = ((2.0, 0.0), (-0.5, 0.0))
    out.append(_case("stream", "NN", 262144 + 77, 128, 32, pairs=b0, rbeta=0.0, chain="slices"))
    out.append(_case("stream", "NT", 262144 + 77, 128, 32, pairs=b0, rbeta=0.0, chain="slices"))
    out.append(_case("stream_no_wt", "NT", 262144 + 77, 128, 64, pairs=b0, rbeta=0.0, ws="zero", chain="slices"))
    out.append(_case("stream", "NT", 262144 + 77, 128, 96, pairs=b0, rbeta=0.0, chain="slices"))   # three K-tiles, B K-contiguous
    out.append(_case("stream", "NN", 131072 + 5, 512, 32, pairs=b0, rbeta=0.0, chain="slices"))
    # LDS-DMA kernel: 256 x 128, 256 x 256, guarded last column tile; the tail geometry; C off the grid (declined)
    for N in (128, 256, 100):
        for trans in ("NN", "NT"):
            out.append(_case("dma", trans, 2048 + 13, N, 64, pairs=b0, rbeta=0.0, chain="slices"))
    out.append(_case("dma_tail", "NN", 256 * (256 + 18) + 100, 256, 64, pairs=b0, rbeta=0.0, chain="slices"))
    out.append(_case("dma_declined", "NN", 2048 + 13, 128, 64, layout="aao", pairs=b0, rbeta=0.0))
    # LDS-DMA TN kernel: both geometries, the K % 64 remainder slab, and A off the grid (the generic kernel's own split)
    tn = ((2.0, 0.0), (2.0, 1.0))
    out.append(_case("dma_tn", "TN", 128, 128, 65536, pairs=tn, chain="rerun"))
    out.append(_case("dma_tn", "TN", 128, 128, 65536 + 17, pairs=tn, chain="rerun"))
    out.append(_case("dma_tn", "TN", 256, 256, 65536, pairs=tn, chain="rerun"))
    out.append(_case("dma_tn_declined", "TN", 128, 128, 65536 + 17, layout="oaa", pairs=tn, chain="rerun"))
    return tuple(out)


CASES = _build_cases()


def case_betas(case):
    """Every beta a case calls gnnx_gemm_f32 with (the path depends on beta == 0): the exact leg's, the rounding leg's, and the
    beta = 0 of the identity and same-chain legs."""
    return sorted({b for _, b in case.pairs} | {case.rbeta, 0.0})


def case_workspace(case):
    return 0 if case.ws == "zero" else gemm_workspace(case.trans[0] == "T", case.trans[1] == "T", case.M, case.N, case.K)


def case_path(case, beta):
    al = [c == "a" for c in case.layout]
    return gemm_path(case.trans[0] == "T", case.trans[1] == "T", case.M, case.N, case.K, beta, al[0], al[1], al[2], case_workspace(case))
