"""CPU half of the gnnx_gemm_f32 contract tests: the shape table of tests/gemm_ref.py reaches every dispatch cell of
csrc/gnnx_gemm.hip (asserted from gemm_ref.gemm_path, cell by cell: a cell the table misses is a failure, and every cell is printed
with the case that reaches it), the restated workspace rule is the library's, and the epilogue's three-rounding arithmetic
(gemm_ref.epilogue_f32) is visible in the bits next to either fused form -- so tests/test_gpu_gemm_contract.py's identity leg turns
red on a build that contracts the epilogue."""
import ctypes as C
import importlib
import itertools

import numpy as np

from tests import gemm_ref as gr
from tests.helpers import pkg, synth  # noqa: F401


def reached():
    """cell -> name of the first case (and beta) whose path holds it."""
    out = {}
    for case in gr.CASES:
        for beta in gr.case_betas(case):
            path = gr.case_path(case, beta)
            kinds = [c.kernel for c in path]
            trans = case.trans
            for c in path:
                keys = []
                if c.kernel == "gemm_kernel":
                    keys.append(("gemm_kernel", c.layout, c.tile, c.vec_a, c.vec_b))
                    if c.splits > 1:
                        keys.append(("split-K", "2" if c.splits == 2 else "a few" if c.splits < 64 else ">= 256" if c.splits >= 256 else "some"))
                        if trans == "TN" and gr.dma_tn_shape_ok(case.M, case.N, case.K - case.K % 64):
                            keys.append(("declined", "gemm_dma_tn_kernel -> gemm_kernel's own split"))
                elif c.kernel == "gemm_stream_kernel":
                    keys.append(("gemm_stream_kernel", c.tile, "B " + ("K-contiguous" if c.layout == "T" else "k-major")))
                    if trans == "NT" and gr.dma_shape_ok(case.M, case.N, case.K) and "transpose_w" not in kinds:
                        keys.append(("declined", "no W^T workspace -> gemm_stream_kernel, gemm_kernel"))
                elif c.kernel == "gemm_dma_kernel":
                    keys.append(("gemm_dma_kernel", c.tile))
                    if kinds.count("gemm_dma_kernel") == 2:
                        keys.append(("gemm_dma_kernel", "launch_dma_with_tail"))
                elif c.kernel == "gemm_dma_tn_kernel":
                    keys.append(("gemm_dma_tn_kernel", c.tile))
                    keys.append(("gemm_dma_tn_kernel", "K % 64 remainder slab" if "gemm_kernel" in kinds else "no remainder slab"))
                elif c.kernel == "splitk_reduce_kernel":
                    keys.append(("splitk_reduce_kernel", "beta != 0" if beta != 0 else "beta == 0"))
                for k in keys:
                    out.setdefault(k, f"{case.name} beta={beta}")
            if (trans[0] == "N" and beta == 0 and case.K > 0 and gr.dma_shape_ok(case.M, case.N, case.K) and case.ws == "full"
                    and "gemm_dma_kernel" not in kinds):
                out.setdefault(("declined", "gemm_dma_kernel (alignment) -> " + ", ".join(kinds)), f"{case.name} beta={beta}")
            if case.K == 0:
                out.setdefault(("K = 0", "beta != 0" if beta != 0 else "beta == 0"), f"{case.name} beta={beta}")
    return out


def required():
    req = [("gemm_kernel", layout, tile, va, vb) for layout in ("NN", "NT", "TN", "TT") for tile in gr.CFG
           for va, vb in itertools.product((False, True), repeat=2)]
    req += [("split-K", "2"), ("split-K", "a few"), ("split-K", ">= 256")]
    req += [("gemm_stream_kernel", "kSquare", "B k-major"), ("gemm_stream_kernel", "kSquare", "B K-contiguous"),
            ("gemm_stream_kernel", "kTall32", "B k-major")]
    req += [("gemm_dma_kernel", t) for t in ("256x256", "256x128", "256x128:NG", "128x128", "launch_dma_with_tail")]
    req += [("gemm_dma_tn_kernel", t) for t in ("256x256", "128x128", "K % 64 remainder slab", "no remainder slab")]
    req += [("declined", "gemm_dma_tn_kernel -> gemm_kernel's own split"), ("declined", "no W^T workspace -> gemm_stream_kernel, gemm_kernel"),
            ("declined", "gemm_dma_kernel (alignment) -> gemm_kernel")]
    req += [("splitk_reduce_kernel", "beta != 0"), ("splitk_reduce_kernel", "beta == 0"), ("K = 0", "beta != 0"), ("K = 0", "beta == 0")]
    return req


def test_table_reaches_every_dispatch_cell():
    got = reached()
    req = required()
    assert len(req) == 48 + 22
    for cell in req:
        print(cell, "<-", got.get(cell, "NOT REACHED"))
    missing = [cell for cell in req if cell not in got]
    assert not missing, f"{len(missing)} cells not reached by gemm_ref.CASES: {missing}"
    names = [c.name for c in gr.CASES]
    assert len(set(names)) == len(names)


def test_every_case_takes_the_path_it_is_named_for():
    """A case whose name says stream / dma / dma_tn holds that kernel on its beta = 0 path; a `declined` one does not; no case of the
    table is refused; the generic cases are one gemm_kernel launch (plus the reduction when split)."""
    for case in gr.CASES:
        for beta in gr.case_betas(case):
            kinds = [c.kernel for c in gr.case_path(case, beta)]
            assert "refused" not in kinds, case.name
            if case.trans[0] == "N":    # the row ranges of a row-parallel product add up to M
                assert sum(c.rows for c in gr.case_path(case, beta) if c.kernel != "transpose_w") == case.M, case.name
        kinds = [c.kernel for c in gr.case_path(case, 0.0)]
        group = case.name.split("-")[0]
        want = {"stream": "gemm_stream_kernel", "stream_no_wt": "gemm_stream_kernel", "dma": "gemm_dma_kernel", "dma_tail": "gemm_dma_kernel",
                "dma_tn": "gemm_dma_tn_kernel"}.get(group)
        if want:
            assert want in kinds, f"{case.name}: {kinds}"
            assert case.chain in ("slices", "rerun")
        if group in ("dma_declined", "dma_tn_declined", "stream_no_wt"):
            assert "gemm_dma_kernel" not in kinds and "gemm_dma_tn_kernel" not in kinds and "transpose_w" not in kinds, f"{case.name}: {kinds}"
        if group in ("generic", "vec", "row", "col", "k0", "gat_er", "gat_dh", "gat_da", "skinny", "splitk"):
            assert [k for k in kinds if k != "splitk_reduce_kernel"] == ["gemm_kernel"], f"{case.name}: {kinds}"
        if len(kinds) > 1:
            assert case.chain is not None, f"{case.name} is served by {kinds} and has no same-chain leg"


def test_table_stays_small():
    """The largest C is below 270 MB and the largest operand about 100 MB; partial sums of {-1, 0, 1} data stay far below 2^24."""
    for case in gr.CASES:
        assert 4 * case.M * case.N <= 272e6 and 4 * max(case.M, case.N) * case.K <= 101e6, case.name
        assert 2 * case.K < 2 ** 24, case.name


def test_dispatch_helpers_at_their_thresholds():
    assert gr.pick_tile(255, 129) == "kWide" and gr.pick_tile(256, 129) == "kTall32" and gr.pick_tile(10 ** 6, 128) == "kSquare"
    assert gr.choose_splits(256, 256, 10_000_000) == 256 and gr.choose_splits(128, 128, 1_000_000) == 512
    assert gr.choose_splits(300, 130, 700) == 2 and gr.choose_splits(7, 2, 515) == 2 and gr.choose_splits(64, 96, 200000) == 512
    assert gr.choose_splits(130, 70, 4099) == 16 and gr.choose_splits(2, 128, 40001) == 156 and gr.choose_splits(130, 130, 130) == 1
    assert gr.dma_shape_ok(2048, 64, 64) and not gr.dma_shape_ok(2047, 64, 64) and not gr.dma_shape_ok(2048, 66, 64)
    assert not gr.dma_shape_ok(2048, 64, 96) and not gr.dma_shape_ok(2048, 60, 64)
    assert gr.dma_tn_shape_ok(128, 256, 65536) and not gr.dma_tn_shape_ok(128, 256, 65536 - 64) and not gr.dma_tn_shape_ok(64, 128, 65536)
    # one workspace byte short of the slabs: refused, whatever else is aligned
    need = gr.gemm_workspace(True, False, 128, 128, 65536)
    assert [c.kernel for c in gr.gemm_path(True, False, 128, 128, 65536, 0.0, True, True, True, need - 1)] == ["refused"]
    assert gr.gemm_path(False, False, 0, 5, 3, 0.0, True, True, True, 0) == [] and gr.gemm_path(False, False, 5, 0, 3, 0.0, True, True, True, 0) == []


def test_workspace_rule_is_the_librarys():
    """gemm_ref.gemm_workspace (choose_splits, dma_shape_ok) against gnnx_gemm_workspace for every case of the table and a sweep of
    shapes around the thresholds: the library answers without a device."""
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module("gnncpp_amd.capi").lib()
    shapes = [(c.M, c.N, c.K) for c in gr.CASES]
    shapes += list(itertools.product((1, 127, 128, 129, 255, 256, 257, 2047, 2048, 70000), (1, 63, 64, 100, 128, 129, 256, 257, 512),
                                     (0, 1, 31, 64, 255, 256, 257, 4099, 65536, 65553, 10 ** 6)))
    b = C.c_size_t(0)
    for M, N, K in shapes:
        for tA, tB in itertools.product((0, 1), repeat=2):
            assert L.gnnx_gemm_workspace(tA, tB, M, N, K, C.byref(b)) == 0
            assert b.value == gr.gemm_workspace(tA, tB, M, N, K), (tA, tB, M, N, K)


def test_epilogue_three_roundings_are_visible_in_the_bits():
    """The rounding leg's alpha = 0.3, beta = -1.7 on seeded uniform data: fl(fl(alpha P) + fl(beta C0)) differs from
    fma(alpha, P, fl(beta C0)) in 33 % of 2^20 elements and from fma(beta, C0, fl(alpha P)) in 29 % (either: 45 %); the bar is 5 % for
    each, three orders above "a handful".  A build that contracts the epilogue into either fused form therefore fails the identity
    leg of the GPU file on about every third element.  The fused forms are emulated through float64: the product of two float32 is
    exact there, and the one double rounding of the sum touches far fewer elements than the bar."""
    n = 1 << 20
    P = synth.uniform_pm1(4001, (n,)) * np.float32(8)
    C0 = synth.uniform_pm1(4002, (n,))
    alpha, beta = np.float32(0.3), np.float32(-1.7)
    three = gr.epilogue_f32(P, C0, alpha, beta)
    assert three.dtype == np.float32
    bc, ap = (beta * C0).astype(np.float32), (alpha * P).astype(np.float32)
    fused_a = (np.float64(alpha) * P.astype(np.float64) + bc.astype(np.float64)).astype(np.float32)
    fused_b = (np.float64(beta) * C0.astype(np.float64) + ap.astype(np.float64)).astype(np.float32)
    share_a, share_b = float((three != fused_a).mean()), float((three != fused_b).mean())
    either = float(((three != fused_a) | (three != fused_b)).mean())
    print(f"differs from fma(alpha, P, fl(beta C0)): {share_a:.4f}; from fma(beta, C0, fl(alpha P)): {share_b:.4f}; either: {either:.4f}")
    assert share_a > 0.05 and share_b > 0.05
    # beta == 0: one rounding, C0 is not read (NaN there must not matter)
    assert np.array_equal(gr.epilogue_f32(P, np.full(n, np.nan, np.float32), alpha, 0.0), ap)
    # exact data: the epilogue is exact whatever the form
    Pi, Ci = np.arange(-8, 8, dtype=np.float32), np.arange(16, dtype=np.float32)
    assert np.array_equal(gr.epilogue_f32(Pi, Ci, -0.5, 0.5), -0.5 * Pi.astype(np.float64) + 0.5 * Ci)
