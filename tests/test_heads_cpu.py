"""CPU-side checks of the multi-head calls: the NumPy restatements tests/heads_ref.py equal the loop of the single-head restatements
over the heads (tests/spmm_ref.py, tests/sddmm_ref.py, tests/edge_softmax_ref.py on slab h / column h) bit for bit -- the one sentence
of the header's contract -- and agree with float64 at the bars of the single-head files: tests.helpers.assert_close with
absum = sum |terms| for the aggregation and the scores (test_spmm_ref_cpu.py, test_sddmm_cpu.py), and for the softmax the forward at
assert_close, the backward at assert_close with the row's absum = sum_p |alpha_p dalpha_p| (test_gpu_edge_softmax.py's bar for the
float64 leg).  The new entry points validate their arguments before any device call."""
import importlib

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import heads_ref as hr
from tests import sddmm_ref as sr
from tests.helpers import assert_close
from tests.spmm_ref import spmm_ref

CELLS = hr.CELLS_CPU + ((1, 12),)


@pytest.fixture(scope="module")
def pattern():
    rowptr, colidx, _ = er.pattern_a()
    return rowptr, colidx, len(rowptr) - 1, er.N_COLS_A, len(colidx)


def operands(pattern, H, D, seed=0):
    _, _, n_rows, n_cols, nnz = pattern
    rng = np.random.default_rng(1000 * H + D + seed)
    u = lambda *shape: rng.uniform(-1, 1, shape).astype(np.float32)  # noqa: E731
    return dict(X=u(n_cols, H * D), L=u(n_rows, H * D), vals=u(nnz, H), bias=u(H * D), y0=u(n_rows, H * D))


@pytest.mark.parametrize("H,D", CELLS)
def test_aggregation_equals_the_loop_over_heads(pattern, H, D):
    rowptr, colidx = pattern[:2]
    op = operands(pattern, H, D)
    for kw in (dict(), dict(bias=op["bias"], relu_out=True), dict(bias=op["bias"], y0=op["y0"])):
        got = hr.spmm_heads_ref(rowptr, colidx, op["X"], op["vals"], H, **kw)
        for h in range(H):
            kh = dict(kw)
            if "bias" in kh:
                kh["bias"] = kh["bias"][h * D:(h + 1) * D]
            if "y0" in kh:
                kh["y0"] = hr.slab(kh["y0"], h, H)
            want = spmm_ref(rowptr, colidx, hr.slab(op["X"], h, H), vals=np.ascontiguousarray(op["vals"][:, h]), **kh)
            assert np.array_equal(got[:, h * D:(h + 1) * D], want), f"head {h} of ({H}, {D}), {sorted(kw)}"
    if H == 1:
        assert np.array_equal(hr.spmm_heads_ref(rowptr, colidx, op["X"], op["vals"], 1), spmm_ref(rowptr, colidx, op["X"], vals=op["vals"][:, 0]))


@pytest.mark.parametrize("H,D", CELLS)
def test_scores_equal_the_loop_over_heads(pattern, H, D):
    rowptr, colidx = pattern[:2]
    op = operands(pattern, H, D)
    got = hr.sddmm_heads_ref(rowptr, colidx, op["L"], op["X"], H)
    assert got.shape == (len(colidx), H)
    for h in range(H):
        assert np.array_equal(got[:, h], sr.sddmm_ref(rowptr, colidx, hr.slab(op["L"], h, H), hr.slab(op["X"], h, H))), f"head {h} of ({H}, {D})"


def softmax_operands(pattern, H, mode):
    _, _, n_rows, n_cols, nnz = pattern
    rng = np.random.default_rng(77 + H)
    s, t = mode in ("scores", "all"), mode in ("terms", "all")
    kw = dict(scores=rng.uniform(-2, 2, (nnz, H)).astype(np.float32) if s else None,
              rowterm=rng.uniform(-2, 2, (n_rows, H)).astype(np.float32) if t else None,
              colterm=rng.uniform(-2, 2, (n_cols, H)).astype(np.float32) if t else None)
    return kw, (1.0 if mode == "scores" else 0.2), rng.uniform(-1, 1, (nnz, H)).astype(np.float32)


def column(kw, h):
    return {k: None if v is None else np.ascontiguousarray(v[:, h]) for k, v in kw.items()}


@pytest.mark.parametrize("mode", ["scores", "terms", "all"])
@pytest.mark.parametrize("H", [1, 3, 8])
def test_softmax_equals_the_loop_over_heads(pattern, H, mode):
    rowptr, colidx = pattern[:2]
    kw, slope, dalpha = softmax_operands(pattern, H, mode)
    alpha, x, m, z = hr.edge_softmax_heads_ref(rowptr, colidx, slope=slope, **kw)
    dt, drow = hr.edge_softmax_heads_bwd_ref(rowptr, colidx, alpha, dalpha, slope=slope, **kw)
    for h in range(H):
        a1, x1, m1, z1 = er.edge_softmax_ref(rowptr, colidx, slope=slope, **column(kw, h))
        assert np.array_equal(alpha[:, h], a1) and np.array_equal(x[:, h], x1) and np.array_equal(m[:, h], m1) and np.array_equal(z[:, h], z1)
        dt1, drow1 = er.edge_softmax_bwd_ref(rowptr, colidx, a1, np.ascontiguousarray(dalpha[:, h]), slope=slope, **column(kw, h))
        assert np.array_equal(dt[:, h], dt1) and np.array_equal(drow[:, h], drow1)
    empty = np.diff(rowptr) == 0
    assert np.isneginf(m[empty]).all() and (z[empty] == 0).all() and (drow[empty] == 0).all()


def test_restatements_vs_float64(pattern):
    rowptr, colidx, n_rows, n_cols, nnz = pattern
    H, D = 4, 6
    op = operands(pattern, H, D)
    rows, cols = er.row_of_entries(rowptr), colidx.astype(np.int64)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    # aggregation
    terms = f64(op["vals"])[:, :, None] * f64(op["X"])[cols].reshape(nnz, H, D)
    ref, absum = np.zeros((n_rows, H, D)), np.zeros((n_rows, H, D))
    np.add.at(ref, rows, terms)
    np.add.at(absum, rows, np.abs(terms))
    ref = ref.reshape(n_rows, H * D) + f64(op["bias"])
    absum = absum.reshape(n_rows, H * D) + np.abs(f64(op["bias"]))
    assert_close(hr.spmm_heads_ref(rowptr, colidx, op["X"], op["vals"], H, bias=op["bias"]), ref, "aggregation", absum=absum)
    # scores
    prod = (f64(op["L"])[rows] * f64(op["X"])[cols]).reshape(nnz, H, D)
    assert_close(hr.sddmm_heads_ref(rowptr, colidx, op["L"], op["X"], H), prod.sum(2), "scores", absum=np.abs(prod).sum(2))
    # softmax, forward and backward
    kw, slope, dalpha = softmax_operands(pattern, 3, "all")
    alpha, _, _, _ = hr.edge_softmax_heads_ref(rowptr, colidx, slope=slope, **kw)
    dt, drow = hr.edge_softmax_heads_bwd_ref(rowptr, colidx, alpha, dalpha, slope=slope, **kw)
    for h in range(3):
        m64 = er.edge_softmax_ref64(rowptr, colidx, n_cols, slope=slope, dalpha=dalpha[:, h], **column(kw, h))
        assert_close(alpha[:, h], m64["alpha"], f"alpha, head {h}")
        assert_close(dt[:, h], m64["dt"], f"dt, head {h}", absum=m64["absum"][rows])
        assert_close(drow[:, h], m64["drowterm"], f"drowterm, head {h}", absum=2 * m64["absum"])


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_argument_validation_without_device(capi):
    """Validation happens before any HIP call, so these return statuses even with no GPU.  The pointers are never dereferenced."""
    import ctypes as C
    L = capi.lib()
    p = C.c_void_p(256)   # a non-null stand-in
    agg = lambda **k: L.gnnx_spmm_csr_heads_f32(*[k.get(n, d) for n, d in (  # noqa: E731
        ("n_rows", 4), ("n_cols", 4), ("H", 2), ("D", 4), ("rowptr", p), ("colidx", p), ("vals", p), ("ldv", 2), ("bias", None), ("X", p),
        ("ldx", 8), ("beta", 0.0), ("relu", 0), ("Y", p), ("ldy", 8), ("stream", None))])
    for bad in (dict(n_rows=-1), dict(n_cols=-1), dict(H=0), dict(D=0), dict(ldv=1), dict(ldx=7), dict(ldy=7), dict(beta=0.5),
                dict(rowptr=None), dict(colidx=None), dict(vals=None), dict(X=None), dict(Y=None)):
        assert agg(**bad) == -1, bad
    assert agg(rowptr=None) == -1 and b"null" in L.gnnx_last_error()
    assert agg(n_rows=0, rowptr=None, Y=None) == 0

    sc = lambda **k: L.gnnx_sddmm_csr_heads_f32(*[k.get(n, d) for n, d in (  # noqa: E731
        ("n_rows", 4), ("n_cols", 4), ("H", 2), ("D", 4), ("nnz", 5), ("rowptr", p), ("colidx", p), ("L", p), ("ldl", 8), ("R", p), ("ldr", 8),
        ("out", p), ("ldo", 2), ("stream", None))])
    for bad in (dict(n_rows=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(H=0), dict(D=-3), dict(ldl=7), dict(ldr=7), dict(ldo=1), dict(rowptr=None),
                dict(colidx=None), dict(L=None), dict(R=None), dict(out=None), dict(n_rows=0)):
        assert sc(**bad) == -1, bad
    assert sc(nnz=0, rowptr=None, colidx=None, L=None, R=None, out=None) == 0

    b = C.c_size_t(0)
    assert L.gnnx_edge_softmax_heads_workspace(100, 1000, 0, C.byref(b)) == -1
    assert L.gnnx_edge_softmax_heads_workspace(100, 1 << 31, 2, C.byref(b)) == -1
    assert L.gnnx_edge_softmax_heads_workspace(100, 1000, 2, None) == -1
    one, eight = C.c_size_t(0), C.c_size_t(0)
    single = C.c_size_t(0)
    n, nnz = 1000, 3_000_000
    assert L.gnnx_edge_softmax_workspace(n, nnz, C.byref(single)) == 0
    assert L.gnnx_edge_softmax_heads_workspace(n, nnz, 1, C.byref(one)) == 0 and one.value == single.value
    assert L.gnnx_edge_softmax_heads_workspace(n, nnz, 8, C.byref(eight)) == 0 and eight.value > one.value

    fwd = lambda **k: L.gnnx_edge_softmax_csr_heads_f32(*[k.get(n, d) for n, d in (  # noqa: E731
        ("n_rows", 4), ("n_cols", 4), ("nnz", 5), ("rowptr", p), ("colidx", p), ("H", 2), ("scores", p), ("lds", 2), ("rowterm", p), ("rs", 4),
        ("colterm", p), ("cs", 4), ("slope", 0.2), ("flags", 0), ("out", p), ("ldo", 2), ("rowmax", None), ("rowsum", None), ("ws", p),
        ("bytes", 1 << 20), ("stream", None))])
    for bad in (dict(n_rows=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(H=0), dict(lds=1), dict(rs=1), dict(cs=1), dict(ldo=1), dict(flags=2),
                dict(rowptr=None), dict(colidx=None), dict(out=None), dict(scores=None, rowterm=None, colterm=None)):
        assert fwd(**bad) == -1, bad
    assert fwd(ws=None) == -4 and fwd(bytes=8) == -4

    bwd = lambda **k: L.gnnx_edge_softmax_bwd_csr_heads_f32(*[k.get(n, d) for n, d in (  # noqa: E731
        ("n_rows", 4), ("n_cols", 4), ("nnz", 5), ("rowptr", p), ("colidx", p), ("H", 2), ("scores", p), ("lds", 2), ("rowterm", p), ("rs", 4),
        ("colterm", p), ("cs", 4), ("slope", 0.2), ("alpha", p), ("lda", 2), ("dalpha", p), ("ldd", 2), ("dt", p), ("ldt", 2), ("drow", p),
        ("drs", 4), ("ws", p), ("bytes", 1 << 20), ("stream", None))])
    for bad in (dict(n_rows=-1), dict(nnz=1 << 31), dict(H=0), dict(lds=1), dict(rs=1), dict(cs=1), dict(lda=1), dict(ldd=1), dict(ldt=1),
                dict(drs=1), dict(rowptr=None), dict(alpha=None), dict(dalpha=None), dict(dt=None)):
        assert bwd(**bad) == -1, bad
    assert bwd(bytes=8) == -4
