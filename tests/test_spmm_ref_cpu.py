"""The yardstick of tests/test_gpu_spmm_dispatch.py held to its own references, and the proof that the width lists of that file
reach every cell of the aggregation's dispatch table (gnnx_spmm.hip: spmm_impl).

  * tests/spmm_ref.py::spmm_ref (float32 NumPy, the header's order) equals the C oracle bit for bit -- forward (rowscale + bias),
    backward (the per-source norm as per-entry values and as a column scale), per-entry values -- on two seeded R-MAT graphs with
    hubs, at one width of 16-byte pieces and one scalar width; beta = 1 and the ReLU epilogue by their definition;
  * modes 1 and 6 (colscale, vals + colscale), which the oracle has no function for, against float64 within the suite's
    condition-aware bar |ref - f64| <= 1e-5 * max(1, sum of |terms|) (tests/helpers.py);
  * the width lists through spmm_cell: every (VEC, G) pair, both edges of every G's range, G = 64 with several and with ragged
    feature tiles.  Trimming a list below that fails here, without a GPU."""
import numpy as np
import pytest

import oracle
from tests.golden_util import same
from tests.helpers import assert_close, synth
from tests.spmm_ref import BF16_UNALIGNED_WIDTHS, UNALIGNED_WIDTHS, VEC1_WIDTHS, VEC4_WIDTHS, spmm_cell, spmm_ref

WIDTHS = (24, 21)   # 16-byte pieces / scalar lanes


@pytest.fixture(scope="module", params=[(3001, 60000, 901), (5000, 120000, 902)], ids=lambda p: f"rmat{p[0]}")
def graph(request):
    n, e, seed = request.param
    src, dst = synth.rmat_edges(seed, n, e)
    rp, ci = oracle.coo_to_csr(src, dst, n)
    rT, cT = oracle.csr_transpose(rp, ci, n)
    s, norm = oracle.degree_norm(rp, ci, n)
    deg = np.diff(rp)
    assert (deg == 0).sum() > 50 and deg.max() > 500 and (deg > 64).sum() > 100, "the graph should have empty rows and hubs"
    return dict(n=n, rp=rp, ci=ci, rT=rT, cT=cT, s=s, norm=norm)


@pytest.mark.parametrize("F", WIDTHS)
def test_restatement_equals_the_oracle_forward(graph, F):
    n, rp, ci, norm = graph["n"], graph["rp"], graph["ci"], graph["norm"]
    H = synth.uniform_pm1(911, (n, F))
    bias = synth.uniform_pm1(912, (F,))
    assert np.array_equal(spmm_ref(rp, ci, H, rowscale=norm, bias=bias), oracle.aggregate_fwd(rp, ci, H, norm, bias))
    assert np.array_equal(spmm_ref(rp, ci, H), oracle.aggregate_fwd(rp, ci, H, None, None))


@pytest.mark.parametrize("F", WIDTHS)
def test_restatement_equals_the_oracle_backward_as_vals_and_as_colscale(graph, F):
    n, rT, cT, norm = graph["n"], graph["rT"], graph["cT"], graph["norm"]
    G = synth.uniform_pm1(913, (n, F))
    want = oracle.aggregate_bwd(rT, cT, G, norm)
    assert same(spmm_ref(rT, cT, G, vals=norm[cT]), want)
    assert same(spmm_ref(rT, cT, G, colscale=norm), want)


@pytest.mark.parametrize("F", WIDTHS)
def test_restatement_equals_the_oracle_per_entry_values(graph, F):
    n, rp, ci = graph["n"], graph["rp"], graph["ci"]
    X = synth.uniform_pm1(914, (n, F))
    vals = synth.uniform_pm1(915, (len(ci),), scale=3.0)
    assert same(spmm_ref(rp, ci, X, vals=vals), oracle.spmm_vals(rp, ci, vals, X))


def test_restatement_accumulate_and_relu_by_definition(graph):
    n, rp, ci, norm = graph["n"], graph["rp"], graph["ci"], graph["norm"]
    F = WIDTHS[1]
    H = synth.uniform_pm1(916, (n, F))
    bias = synth.uniform_pm1(917, (F,))
    y0 = synth.uniform_pm1(918, (n, F))
    base = oracle.aggregate_fwd(rp, ci, H, norm, bias)
    acc = spmm_ref(rp, ci, H, rowscale=norm, bias=bias, y0=y0)
    assert acc.dtype == np.float32 and np.array_equal(acc, y0 + base)          # beta = 1: Y + (...), one rounded add
    got = spmm_ref(rp, ci, H, rowscale=norm, bias=bias, y0=y0, relu_out=True)
    assert np.array_equal(got, np.maximum(acc, np.float32(0)))
    assert (acc < 0).sum() > 1000 and float(got.min()) == 0.0                   # the ReLU had something to do
    assert np.array_equal(spmm_ref(rp, ci, H, rowscale=norm, bias=bias, relu_out=True), np.maximum(base, np.float32(0)))


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("with_vals", [False, True], ids=["mode1", "mode6"])
def test_restatement_colscale_modes_vs_float64(graph, F, with_vals):
    """colscale (mode 1) and vals + colscale (mode 6) on CSR(A) and CSR(A^T): the oracle has no such function, so float64 holds them."""
    n, s, norm = graph["n"], graph["s"], graph["norm"]
    X = synth.uniform_pm1(919, (n, F))
    bias = synth.uniform_pm1(920, (F,))
    for rp, ci in ((graph["rp"], graph["ci"]), (graph["rT"], graph["cT"])):
        vals = synth.uniform_pm1(921, (len(ci),)) if with_vals else None
        rowscale = norm if with_vals else s
        got = spmm_ref(rp, ci, X, vals=vals, colscale=s, rowscale=rowscale, bias=bias)
        w = s[ci].astype(np.float64) * (vals.astype(np.float64) if with_vals else 1.0)
        rows = np.repeat(np.arange(n), np.diff(rp))
        ref, absum = np.zeros((n, F)), np.zeros((n, F))
        np.add.at(ref, rows, w[:, None] * X[ci].astype(np.float64))
        np.add.at(absum, rows, np.abs(w)[:, None] * np.abs(X[ci]).astype(np.float64))
        rs = rowscale.astype(np.float64)[:, None]
        ref = ref * rs + bias.astype(np.float64)[None, :]
        absum = absum * np.abs(rs) + np.abs(bias).astype(np.float64)[None, :]
        assert_close(got, ref, "restated colscale mode", absum=absum)


def test_dispatch_rule_on_the_documented_widths():
    # gnnx_spmm.hip's header: 64 lanes at F = 256, two rows per wavefront at F = 128 / 100; the streaming kernel at F > 64
    assert spmm_cell(256) == (4, 64, "stream", 1) and spmm_cell(128) == (4, 32, "stream", 1) and spmm_cell(100) == (4, 32, "stream", 1)
    assert spmm_cell(64) == (4, 16, "rows", 1) and spmm_cell(20) == (4, 8, "rows", 1) and spmm_cell(16) == (4, 4, "rows", 1)
    assert spmm_cell(33) == (1, 64, "stream", 1) and spmm_cell(7) == (1, 8, "rows", 1) and spmm_cell(1) == (1, 4, "rows", 1)
    assert spmm_cell(70) == (1, 64, "stream", 2) and spmm_cell(516) == (4, 64, "stream", 3)
    assert spmm_cell(32, aligned=False) == (1, 32, "stream", 1) and spmm_cell(256, aligned=False) == (1, 64, "stream", 4)


def test_width_lists_reach_every_cell_of_the_dispatch_table():
    assert all(F % 4 == 0 for F in VEC4_WIDTHS) and all(F % 4 != 0 for F in VEC1_WIDTHS)
    cells = {}
    for F in VEC4_WIDTHS + VEC1_WIDTHS:
        vec, G, kernel, tiles = spmm_cell(F)
        cells.setdefault((vec, G), []).append((F, tiles))
        assert kernel == ("stream" if G >= 32 else "rows")
    assert set(cells) == {(v, G) for v in (1, 4) for G in (4, 8, 16, 32, 64)}, "a (VEC, G) pair is not reached"
    for vec in (1, 4):
        wide = cells[(vec, 64)]
        assert any(t >= 2 for _, t in wide), f"VEC {vec}: no G = 64 width with more than one feature tile"
        assert any(t >= 2 and F % (64 * vec) for F, t in wide), f"VEC {vec}: no G = 64 width with a ragged last tile"
    # both edges of every G's range: the largest width of one G and the smallest of the next.  On scalar lanes the largest width of a
    # range is a multiple of 4, which only an unaligned call brings there; the largest an aligned call brings is one below
    for vec, edges in ((4, ((16, 20), (32, 36), (64, 68), (128, 132))), (1, ((4, 5), (8, 9), (16, 17), (32, 33)))):
        widths = VEC4_WIDTHS if vec == 4 else VEC1_WIDTHS
        assert min(widths) == vec, f"VEC {vec}: the narrowest width is missing"
        for lo, hi in edges:
            assert hi in widths and (lo in widths if vec == 4 else lo in UNALIGNED_WIDTHS and lo - 1 in widths), \
                f"VEC {vec}: the edge {lo} | {hi} is not in the lists"
            top, above = spmm_cell(lo, aligned=vec == 4), spmm_cell(hi)
            assert top[0] == above[0] == vec and above[1] == 2 * top[1] and (vec == 4 or spmm_cell(lo - 1)[:2] == top[:2])
    # the alignment fallback: multiples of 4 on scalar lanes -- the row kernel, the streaming kernel at G = 32 and at G = 64 with one
    # and with several tiles (the latter also puts spmm_hub_kernel<1> on more than one 64-feature slab)
    un = {F: spmm_cell(F, aligned=False) for F in UNALIGNED_WIDTHS}
    assert all(F % 4 == 0 and c[0] == 1 for F, c in un.items())
    assert {c[1] for c in un.values()} == {4, 8, 16, 32, 64} and {c[2] for c in un.values()} == {"rows", "stream"}
    assert any(c[1] == 64 and c[3] == 1 for c in un.values()) and any(c[1] == 64 and c[3] >= 2 for c in un.values())
    b16 = {F: spmm_cell(F, aligned=False) for F in BF16_UNALIGNED_WIDTHS}
    assert all(F % 4 == 0 for F in b16) and {c[1] for c in b16.values()} >= {32, 64} and any(c[3] >= 2 for c in b16.values())
