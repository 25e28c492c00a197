"""CPU-side checks of the edge-score (SDDMM) work: the NumPy restatement tests/sddmm_ref.py is right (against float64), its order is
visible in the bits (so the GPU's bit-equality tests discriminate it), the width list covers every lane group, and the three new
C-ABI entry points are declared, exported, bound and refuse bad arguments before they touch a device.  The numerics on the device are
tests/test_gpu_sddmm.py and tests/test_gpu_link.py.

Bar of the float64 comparison: tests.helpers.assert_close with absum = sum_f |a_f b_f|, i.e. 1e-5 * max(1, |ref|, absum).  The plain
1e-5 * max(1, |ref|) bar does not fit a 1024-term dot product of O(1) operands whose result cancels: the restatement alone reaches
1.02 of it at F = 1024, while its error stays within 2.3 * 2^-24 * absum at every width -- under 0.02 of the absum-aware bar."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest

from tests import sddmm_ref as sr
from tests.helpers import assert_close, pkg  # noqa: F401

NEW_SYMBOLS = ["gnnx_sddmm_csr_f32", "gnnx_csr_transpose_map", "gnnx_bce_logits_workspace", "gnnx_bce_logits_f32"]


@pytest.fixture(scope="module")
def case():
    """A random 300-row rectangular pattern and the operand seeds shared by the width tests."""
    rowptr, colidx = sr.random_csr(5, 300, 217, 4000)
    return dict(rowptr=rowptr, colidx=colidx, rows=sr.row_of_entries(rowptr), n_rows=300, n_cols=217)


def operands(case, F):
    rng = np.random.default_rng(1000 + F)
    L = rng.uniform(-1, 1, (case["n_rows"], F)).astype(np.float32)
    R = rng.uniform(-1, 1, (case["n_cols"], F)).astype(np.float32)
    return L, R


def test_width_list_reaches_every_lane_group_and_chunk_count():
    cells = {sr.lane_group(F)[1:] for F in sr.WIDTHS}
    assert {g for g, _ in cells} == {1, 2, 4, 8, 16, 32, 64}
    assert {c for g, c in cells if g == 64} == {1, 2, 3, 4}
    assert all(c == 1 for g, c in cells if g < 64)
    assert any(sr.lane_group(F)[0] < sr.lane_group(F)[1] for F in sr.WIDTHS)          # idle lanes
    assert any(F % 4 and F > 4 for F in sr.WIDTHS)                                    # a ragged last chunk
    assert sr.lane_group(4) == (1, 1, 1) and sr.lane_group(5) == (2, 2, 1) and sr.lane_group(256) == (64, 64, 1)
    assert sr.lane_group(257) == (65, 64, 2) and sr.lane_group(1024) == (256, 64, 4) and sr.lane_group(132) == (33, 64, 1)


@pytest.mark.parametrize("F", sr.WIDTHS)
def test_sddmm_ref_vs_float64(case, F):
    L, R = operands(case, F)
    rng = np.random.default_rng(7)
    rs = rng.uniform(0.5, 2.0, case["n_rows"]).astype(np.float32)
    cs = rng.uniform(-2.0, -0.5, case["n_cols"]).astype(np.float32)
    rows, cols = case["rows"], case["colidx"].astype(np.int64)
    terms = L.astype(np.float64)[rows] * R.astype(np.float64)[cols]
    dot64, absum = terms.sum(1), np.abs(terms).sum(1)
    got = sr.sddmm_ref(case["rowptr"], case["colidx"], L, R)
    assert got.dtype == np.float32 and got.shape == dot64.shape
    assert_close(got, dot64, f"sddmm_ref F={F}", absum=absum)
    assert np.abs(got.astype(np.float64) - dot64).max() <= 2.3 * 2.0 ** -24 * absum.max()
    scale = rs.astype(np.float64)[rows] * cs.astype(np.float64)[cols]
    got_s = sr.sddmm_ref(case["rowptr"], case["colidx"], L, R, rowscale=rs, colscale=cs)
    assert_close(got_s, dot64 * scale, f"sddmm_ref scaled F={F}", absum=absum * np.abs(scale))
    # the scales are separately rounded multiplies applied to the unscaled result's bits, row scale first
    assert np.array_equal(got_s, (got * rs[rows]) * cs[cols])
    assert np.array_equal(sr.sddmm_ref(case["rowptr"], case["colidx"], L, R, rowscale=rs), got * rs[rows])
    assert np.array_equal(sr.sddmm_ref(case["rowptr"], case["colidx"], L, R, colscale=cs), got * cs[cols])


@pytest.mark.parametrize("F", [F for F in sr.WIDTHS if F >= 8])
def test_lane_group_order_is_visible_in_the_bits(case, F):
    """More than a quarter of the entries differ from the one-accumulator f-ascending sum: a kernel in another order fails torch.equal."""
    L, R = operands(case, F)
    rows, cols = case["rows"], case["colidx"].astype(np.int64)
    differ = float((sr.sddmm_ref(case["rowptr"], case["colidx"], L, R) != sr.dots_ascending(L[rows], R[cols])).mean())
    assert differ > 0.25, f"F={F}: only {differ:.0%} of the entries tell the two orders apart"


def test_narrow_rows_are_the_plain_sum():
    """F <= 4: one lane, one chunk -- the ascending sum itself."""
    rng = np.random.default_rng(3)
    for F in (1, 3, 4):
        A, B = rng.uniform(-1, 1, (500, F)).astype(np.float32), rng.uniform(-1, 1, (500, F)).astype(np.float32)
        assert np.array_equal(sr.dots_in_lane_order(A, B), sr.dots_ascending(A, B))


def test_hand_written_3x3():
    """A = [[a, b, .], [., ., c], [d, ., e]] (positions 0..4), A^T = [[a, ., d], [b, ., .], [., c, e]]."""
    rowptr, colidx = np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 2, 0, 2], np.int32)
    rowptr_t, colidx_t = sr.transpose_csr(rowptr, colidx, 3)
    assert rowptr_t.tolist() == [0, 2, 3, 5] and colidx_t.tolist() == [0, 2, 0, 1, 2]
    assert sr.transpose_map_ref(rowptr, colidx, rowptr_t, colidx_t).tolist() == [0, 3, 1, 2, 4]
    with pytest.raises(KeyError):   # entry (1, 0) of the "transpose" moved to (1, 1): A stores no (1, 1)
        sr.transpose_map_ref(rowptr, colidx, rowptr_t, np.array([0, 2, 1, 1, 2], np.int32))
    L = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    R = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    assert sr.sddmm_ref(rowptr, colidx, L, R).tolist() == [1, 2, 7, 5, 11]
    rs, cs = np.array([2, 3, 0.5], np.float32), np.array([1, 10, 100], np.float32)
    assert sr.sddmm_ref(rowptr, colidx, L, R, rowscale=rs).tolist() == [2, 4, 21, 2.5, 5.5]
    assert sr.sddmm_ref(rowptr, colidx, L, R, colscale=cs).tolist() == [1, 20, 700, 5, 1100]
    assert sr.sddmm_ref(rowptr, colidx, L, R, rowscale=rs, colscale=cs).tolist() == [2, 40, 2100, 2.5, 550]
    assert sr.sddmm_ref(rowptr, colidx, np.zeros((3, 0), np.float32), np.zeros((3, 0), np.float32)).tolist() == [0] * 5


def test_bce_ref_closed_forms():
    x = np.array([0.0, 0.0, 100.0, 100.0, -100.0, -100.0])
    y = np.array([0.0, 1.0, 1.0, 0.0, 0.0, 1.0])
    want = np.array([np.log(2), np.log(2), np.exp(-100), 100 + np.exp(-100), np.exp(-100), 100 + np.exp(-100)])
    loss, g = sr.bce_logits_ref64(x, y)
    assert np.isfinite(loss) and abs(loss - want.sum() / 6) <= 1e-12 * want.sum()
    assert np.allclose(g, [0.5, -0.5, -np.exp(-100), 1.0, np.exp(-100), -1.0], rtol=1e-12, atol=1e-15)
    assert abs(sr.bce_logits_ref64(x, y, n_total=12)[0] - loss / 2) <= 1e-15
    assert abs(sr.bce_logits_ref64(np.array([0.3]), np.array([0.25]))[0] - (np.log1p(np.exp(0.3)) - 0.075)) <= 1e-15   # a soft label


# ------------------------------------------------------------------ the library: built, exported, bound, argument checks
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_entry_points_are_declared_exported_and_bound(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in declared, f"include/gnnx.h does not declare {n}"
        assert hasattr(L, n), f"libgnnx_hip.so does not export {n}"
        assert n in capi._SIGS, f"capi.py has no signature for {n}"
    header = open(capi.HEADER_PATH).read()
    block = header[header.index("edge scores (SDDMM)"):header.index("int gnnx_sddmm_csr_f32(")]
    for words in ("Q = ceil(F/4)", "smallest power of two", "capped at 64", "acc_l = acc_l + acc_{l xor s}", "dot_p = acc_0",
                  "dL/dvals = gnnx_sddmm_csr_f32(L = G, R = X, rowscale, colscale)", "operation.h:516-523"):
        assert words in block, words


def test_argument_validation_without_device(capi):
    """Null pointers, negative sizes and ld < F are GNNX_ERR_INVALID_ARG (-1) before any device call."""
    L = capi.lib()
    p = C.c_void_p(4096)   # a non-null placeholder: every call below must return before it would be read
    sddmm, tmap, bce = L.gnnx_sddmm_csr_f32, L.gnnx_csr_transpose_map, L.gnnx_bce_logits_f32
    ok = dict(n_rows=3, n_cols=3, F=8, nnz=5, rowptr=p, colidx=p, L=p, ldl=8, R=p, ldr=8, out=p)

    def call_sddmm(**kw):
        a = dict(ok, **kw)
        return sddmm(a["n_rows"], a["n_cols"], a["F"], a["nnz"], a["rowptr"], a["colidx"], a["L"], a["ldl"], a["R"], a["ldr"], None, None,
                     a["out"], None)

    for bad in (dict(rowptr=None), dict(colidx=None), dict(L=None), dict(R=None), dict(out=None), dict(n_rows=-1), dict(n_cols=-1),
                dict(F=-1), dict(nnz=-1), dict(ldl=7), dict(ldr=7)):
        assert call_sddmm(**bad) == -1, bad
    assert call_sddmm(nnz=0, colidx=None, out=None, L=None, R=None) == 0            # nothing to score: no launch

    assert tmap(3, 3, 5, None, p, p, p, p, None) == -1
    assert tmap(3, 3, 5, p, p, None, p, p, None) == -1
    assert tmap(3, 3, 5, p, None, p, p, p, None) == -1
    assert tmap(3, 3, 5, p, p, p, None, p, None) == -1
    assert tmap(3, 3, 5, p, p, p, p, None, None) == -1
    assert tmap(-1, 3, 5, p, p, p, p, p, None) == -1
    assert tmap(3, -1, 5, p, p, p, p, p, None) == -1
    assert tmap(3, 3, -1, p, p, p, p, p, None) == -1

    b = C.c_size_t(0)
    assert L.gnnx_bce_logits_workspace(10, C.byref(b)) == 0 and b.value > 0
    assert L.gnnx_bce_logits_workspace(-1, C.byref(b)) == -1
    assert L.gnnx_bce_logits_workspace(10, None) == -1
    assert bce(p, p, 0, 0, p, p, p, b.value, None) == -1                             # an empty list is an error, never a NaN loss
    assert "empty" in L.gnnx_last_error().decode()
    assert bce(p, p, -1, 5, p, p, p, b.value, None) == -1
    assert bce(None, p, 5, 5, p, p, p, b.value, None) == -1
    assert bce(p, None, 5, 5, p, p, p, b.value, None) == -1
    assert bce(p, p, 5, 4, p, p, p, b.value, None) == -1                             # n_total < n


def test_python_layer_offers_the_link_api(capi):
    ops = importlib.import_module("gnncpp_amd.ops")
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(ops.sddmm) == ["rowptr", "colidx", "L", "R", "rowscale", "colscale", "out"]
    assert sig(ops.spmm_vals_grad) == ["rowptr", "colidx", "G", "X", "rowscale", "colscale"]
    assert sig(ops.csr_transpose_map) == ["rowptr", "colidx", "rowptr_t", "colidx_t"]
    assert sig(ops.bce_logits) == ["scores", "target", "want_grad", "n_total", "grad_out"]
    assert sig(ops.EdgeSet.from_pairs) == ["src", "dst", "label", "n"]
    doc = ops.EdgeSet.from_pairs.__doc__
    assert "BEFORE" in doc and "rmat_edges(seed, n, k, a=.25, b=.25, c=.25)" in doc
    assert sig(ops.GcnStack.link_scores) == ["self", "X", "edges"]
    assert sig(ops.GcnStack.link_train_step) == ["self", "X", "edges", "lr", "weight_decay"]
