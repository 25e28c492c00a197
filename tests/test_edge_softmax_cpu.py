"""CPU-side checks of the edge softmax: the NumPy restatement tests/edge_softmax_ref.py is right (its row order against float64 at the
derived chain bound, its backward against float64 autograd), the row order is visible in the bits (so the GPU's bit-equality tests
discriminate it), and the three new C-ABI entry points are declared, exported, bound and refuse bad arguments before they touch a
device.  The numerics on the device are tests/test_gpu_edge_softmax.py and tests/test_gpu_gat.py.

Bars.  Row order: |sum - float64| <= chain_bound(d) * 2^-24 * sum |v|, chain_bound(d) = ceil(min(d, S) / G) + log2 G + ceil(d / S), the
longest chain of additions an entry goes through (each addition is off by at most 2^-24 of its result, which never exceeds
sum |v|).  Backward: tests.helpers.assert_close with absum = sum_p |alpha_p dalpha_p| of the entry's row -- dt_p = alpha_p (dalpha_p -
dot_i) inherits the row sum's error times alpha_p <= 1; for drowterm the summands obey sum_p |de_p| <= 2 absum."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests.helpers import assert_close, pkg  # noqa: F401

NEW_SYMBOLS = ["gnnx_edge_softmax_workspace", "gnnx_edge_softmax_csr_f32", "gnnx_edge_softmax_bwd_csr_f32"]
ORDER_LENGTHS = list(range(2, 131)) + [255, 256, 257, 1000, 4095, 4096, 4097, 8192, 8193, 12293]


def softmax_like(rng, m, d):
    """m rows of exp(e - max), e uniform in +-6: what the forward's row sum adds."""
    e = rng.uniform(-6, 6, (m, d)).astype(np.float32)
    return np.exp(e - e.max(1, keepdims=True)).astype(np.float32)


def test_lane_counts_and_hand_written_sums():
    assert [er.lanes_of(d) for d in (0, 1, 2, 3, 4, 5, 8, 9, 33, 64, 65, 4096)] == [1, 1, 2, 4, 4, 8, 8, 16, 64, 64, 64, 64]
    assert [er.chain_bound(d) for d in (1, 2, 64, 65, 4096, 4097, 12293)] == [2, 3, 8, 9, 71, 72, 74]
    f = np.float32
    big, one = f(2 ** 24), f(1)
    # d = 3, G = 4: lanes [a, b, c, 0] -> (a + b) + (c + 0); sequentially 2^24 + 1 + 1 stays 2^24, the butterfly order too: a + b first
    assert er.sum_equal_rows(np.array([[big, one, one]], f))[0] == big
    # d = 4, G = 4: (a + b) + (c + d): with a = 2^24, c = d = 1 the pair 1 + 1 = 2 survives
    assert er.sum_equal_rows(np.array([[big, f(0), one, one]], f))[0] == big + f(2)
    assert er.sum_ascending(np.array([[big, f(0), one, one]], f))[0] == big
    # d = 65, G = 64: lane 0 adds v_0 + v_64 before the butterfly
    v = np.zeros((1, 65), f)
    v[0, 0], v[0, 1], v[0, 64] = big, one, one
    assert er.sum_equal_rows(v)[0] == big            # (2^24 + 1) rounds down, then + 1 rounds down again
    v = np.zeros((1, 65), f)
    v[0, 0], v[0, 2], v[0, 3] = big, one, one        # lanes 2 and 3 meet at s = 1: 1 + 1 = 2 reaches lane 0 whole at s = 2
    assert er.sum_equal_rows(v)[0] == big + f(2) and er.sum_ascending(v)[0] == big
    # d = S + 1: the second segment is the last entry alone
    v = np.ones((1, er.S + 1), f)
    assert er.sum_equal_rows(v)[0] == f(er.S + 1)
    rowptr = np.array([0, 0, 3, 3, 4], np.int64)
    assert er.row_sum_in_order(np.array([1, 2, 3, 4], f), rowptr).tolist() == [0, 6, 0, 4]
    assert np.signbit(er.row_sum_in_order(np.array([-0.0], f), np.array([0, 1, 1]))).tolist() == [False, False]   # +0 + -0 = +0; empty: +0


def test_row_order_vs_float64_at_the_chain_bound():
    rng = np.random.default_rng(11)
    worst = 0.0
    for d in ORDER_LENGTHS:
        V = softmax_like(rng, 8, d)
        got = er.sum_equal_rows(V).astype(np.float64)
        exact, absum = V.astype(np.float64).sum(1), np.abs(V).astype(np.float64).sum(1)
        rel = np.abs(got - exact) / (2.0 ** -24 * absum)
        worst = max(worst, float(rel.max()))
        assert rel.max() <= er.chain_bound(d), f"d={d}: {rel.max():.2f} * 2^-24 * sum|v| against the bound {er.chain_bound(d)}"
    print(f"worst error of the row order over {len(ORDER_LENGTHS)} lengths: {worst:.2f} * 2^-24 * sum|v|")


@pytest.mark.parametrize("d", [8, 9, 16, 31, 33, 63, 64, 65, 127, 256, 257, 4095, 4096, 4097, 8193, 12293])
def test_row_order_is_visible_in_the_bits(d):
    """The restated sum differs from the one-accumulator ascending sum in at least a fifth of the rows for 8 <= d < 64 and half of them
    from 64 on: a kernel that adds in another order fails np.array_equal."""
    V = softmax_like(np.random.default_rng(100 + d), 200, d)
    differ = float((er.sum_equal_rows(V) != er.sum_ascending(V)).mean())
    print(f"d={d}: {differ:.0%} of 200 rows tell the two orders apart")
    assert differ >= (0.2 if d < 64 else 0.5), f"d={d}: only {differ:.0%}"


def test_row_sum_of_a_pattern_matches_the_equal_length_form():
    rowptr, colidx, lengths = er.pattern_a()
    assert lengths[0] == 0 and lengths[-1] == 0 and set(er.LENGTHS_A) <= set(lengths.tolist())
    assert int(rowptr[-1]) == len(colidx) and colidx.max() < er.N_COLS_A
    assert all(np.all(np.diff(colidx[rowptr[i]:rowptr[i + 1]]) > 0) for i in range(len(lengths)))
    v = np.random.default_rng(3).uniform(0, 1, len(colidx)).astype(np.float32)
    got = er.row_sum_in_order(v, rowptr)
    for i in (int(np.argmax(lengths)), int(np.nonzero(lengths == 33)[0][0]), int(np.nonzero(lengths == 4097)[0][0])):
        assert got[i] == er.sum_equal_rows(v[None, rowptr[i]:rowptr[i + 1]])[0]
    assert np.all(got[lengths == 0] == 0) and not np.signbit(got[lengths == 0]).any()


def operands(rowptr, colidx, n_cols, seed, signs=True):
    rng = np.random.default_rng(seed)
    n_rows, nnz = len(rowptr) - 1, len(colidx)
    lo = -2.0 if signs else 0.1
    return dict(scores=rng.uniform(lo, 2, nnz).astype(np.float32), rowterm=rng.uniform(lo, 2, n_rows).astype(np.float32),
                colterm=rng.uniform(lo, 2, n_cols).astype(np.float32), dalpha=rng.uniform(-1, 1, nnz).astype(np.float32))


@pytest.mark.parametrize("mode", ["scores", "terms", "all"])
@pytest.mark.parametrize("slope", [1.0, 0.2])
def test_restatements_vs_float64_autograd(mode, slope):
    """Forward and backward restatements, and the float64 NumPy model the GPU tests use, against torch's float64 autograd."""
    import torch
    rowptr, colidx, _ = er.pattern_a()
    n_cols = er.N_COLS_A
    op = operands(rowptr, colidx, n_cols, 5)
    kw = dict(scores=op["scores"] if mode != "terms" else None, rowterm=op["rowterm"] if mode != "scores" else None,
              colterm=op["colterm"] if mode != "scores" else None)
    rows = torch.from_numpy(er.row_of_entries(rowptr))
    cols = torch.from_numpy(colidx.astype(np.int64))
    n_rows = len(rowptr) - 1
    leaf = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in kw.items() if v is not None}
    t = torch.zeros(len(colidx), dtype=torch.float64)
    if "scores" in leaf:
        t = t + leaf["scores"]
    if "rowterm" in leaf:
        t = t + leaf["rowterm"][rows]
    if "colterm" in leaf:
        t = t + leaf["colterm"][cols]
    e = torch.nn.functional.leaky_relu(t, float(np.float32(slope)))
    m = torch.full((n_rows,), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows, e.detach(), "amax")
    x = torch.exp(e - m[rows])
    alpha64 = x / torch.zeros(n_rows, dtype=torch.float64).index_add(0, rows, x)[rows]
    t.retain_grad()
    (alpha64 * torch.from_numpy(op["dalpha"].astype(np.float64))).sum().backward()

    model = er.edge_softmax_ref64(rowptr, colidx, n_cols, slope=slope, dalpha=op["dalpha"], **kw)
    assert np.abs(model["alpha"] - alpha64.detach().numpy()).max() <= 1e-14
    assert np.abs(model["dt"] - t.grad.numpy()).max() <= 1e-13
    if "rowterm" in leaf:
        assert np.abs(model["drowterm"] - leaf["rowterm"].grad.numpy()).max() <= 1e-12
        assert np.abs(model["dcolterm"] - leaf["colterm"].grad.numpy()).max() <= 1e-12

    alpha, x32, m32, z32 = er.edge_softmax_ref(rowptr, colidx, slope=slope, **kw)
    assert alpha.dtype == np.float32
    assert_close(alpha, model["alpha"], f"forward restatement {mode} slope {slope}")
    assert np.array_equal(alpha, er.edge_softmax_from_x(x32, z32, rowptr)) and np.array_equal(z32, er.row_sum_in_order(x32, rowptr))
    assert np.array_equal(m32, er.row_max(er.leaky(er.pre_activation(rowptr, colidx, **kw), slope), rowptr))
    dt, drow = er.edge_softmax_bwd_ref(rowptr, colidx, alpha, op["dalpha"], slope=slope, **kw)
    assert dt.dtype == np.float32 and drow.dtype == np.float32
    ent = er.row_of_entries(rowptr)
    assert_close(dt, model["dt"], f"dt {mode} slope {slope}", absum=model["absum"][ent])
    assert_close(drow, model["drowterm"], f"drowterm {mode} slope {slope}", absum=2 * model["absum"])
    tt = er.pre_activation(rowptr, colidx, **kw)
    assert (tt > 0).any() and (tt < 0).any(), "both branches of the mask must occur"


def test_pre_activation_order_and_leaky():
    rowptr, colidx = np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32)
    f = np.float32
    s, r, c = np.array([2 ** 24, 1, -4], f), np.array([1, 2], f), np.array([1, -1], f)
    # (scores + rowterm) + colterm: (2^24 + 1) rounds to 2^24, + 1 again 2^24 -- not 2^24 + (1 + 1)
    assert er.pre_activation(rowptr, colidx, s, r, c).tolist() == [2 ** 24, 1.0, -3.0]
    assert er.pre_activation(rowptr, colidx, None, r, c).tolist() == [2.0, 0.0, 1.0]
    assert er.pre_activation(rowptr, colidx, s, None, None).tolist() == s.tolist()
    assert er.leaky(np.array([2, 0, -3], f), 0.5).tolist() == [2.0, 0.0, -1.5]
    assert np.array_equal(er.leaky(np.array([2, -3], f), 1.0), np.array([2, -3], f))


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
    block = header[header.index("edge softmax ---"):header.index("int gnnx_edge_softmax_workspace(")]
    for words in ("S = 4096", "smallest power of two with G >= d, capped at 64", "acc_l = acc_l + acc_{l xor s}", "((seg_0 + seg_1) + seg_2)",
                  "x_p / z_i", "de_p  = alpha_p * (dalpha_p - dot_i)", "gnnx_csr_rowsum_f32(rowptr_t, vals = dt[map_t])",
                  "GNNX_EDGE_SOFTMAX_UNNORMALISED"):
        assert words in block, words


def test_argument_validation_without_device(capi):
    """Null pointers, negative sizes, nnz >= 2^31 and three NULL operands are GNNX_ERR_INVALID_ARG (-1) before any device call; a
    small workspace is GNNX_ERR_WORKSPACE (-4), also before any device call."""
    L = capi.lib()
    p = C.c_void_p(4096)   # a non-null placeholder: every call below must return before it would be read
    b = C.c_size_t(0)
    assert L.gnnx_edge_softmax_workspace(1000, 10000, C.byref(b)) == 0 and b.value > 0
    small = b.value
    assert L.gnnx_edge_softmax_workspace(1000, 10_000_000, C.byref(b)) == 0 and b.value > small
    assert L.gnnx_edge_softmax_workspace(0, 0, C.byref(b)) == 0
    assert L.gnnx_edge_softmax_workspace(-1, 10, C.byref(b)) == -1
    assert L.gnnx_edge_softmax_workspace(10, -1, C.byref(b)) == -1
    assert L.gnnx_edge_softmax_workspace(10, 1 << 31, C.byref(b)) == -1
    assert L.gnnx_edge_softmax_workspace(10, 10, None) == -1
    assert L.gnnx_edge_softmax_workspace(1000, 10000, C.byref(b)) == 0
    ok = dict(n_rows=1000, n_cols=1000, nnz=10000, rowptr=p, colidx=p, scores=p, rowterm=p, rs=1, colterm=p, cs=1, out=p, alpha=p, dalpha=p,
              dt=p, ws=p, wsb=b.value, flags=0)

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.gnnx_edge_softmax_csr_f32(a["n_rows"], a["n_cols"], a["nnz"], a["rowptr"], a["colidx"], a["scores"], a["rowterm"], a["rs"],
                                           a["colterm"], a["cs"], 0.2, a["flags"], a["out"], None, None, a["ws"], a["wsb"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return L.gnnx_edge_softmax_bwd_csr_f32(a["n_rows"], a["n_cols"], a["nnz"], a["rowptr"], a["colidx"], a["scores"], a["rowterm"], a["rs"],
                                               a["colterm"], a["cs"], 0.2, a["alpha"], a["dalpha"], a["dt"], None, a["ws"], a["wsb"], None)

    common = (dict(rowptr=None), dict(colidx=None), dict(n_rows=-1), dict(n_cols=-1), dict(nnz=-1), dict(nnz=1 << 31),
              dict(scores=None, rowterm=None, colterm=None), dict(rs=0), dict(cs=-2), dict(n_rows=0), dict(n_cols=0))
    for bad in common + (dict(out=None), dict(flags=2)):
        assert fwd(**bad) == -1, bad
    for bad in common + (dict(alpha=None), dict(dalpha=None), dict(dt=None)):
        assert bwd(**bad) == -1, bad
    assert fwd(scores=None, rowterm=None, colterm=None) == -1 and "all null" in L.gnnx_last_error().decode()
    for call in (fwd, bwd):
        assert call(wsb=ok["wsb"] - 1) == -4
        assert call(ws=None) == -4
        assert call(n_rows=0, n_cols=0, nnz=0, ws=None, wsb=0) == 0          # no rows: nothing to write, no launch


def test_python_layer_offers_the_attention_api(capi):
    ops = importlib.import_module("gnncpp_amd.ops")
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(ops.edge_softmax) == ["rowptr", "colidx", "scores", "rowterm", "colterm", "negative_slope", "unnormalised", "want_stats"]
    assert sig(ops.edge_softmax_bwd)[:8] == ["rowptr", "colidx", "alpha", "dalpha", "scores", "rowterm", "colterm", "negative_slope"]
    assert sig(ops.GatStack.__init__)[:5] == ["self", "g", "dims", "negative_slope", "seed"]
    assert inspect.signature(ops.GatStack.__init__).parameters["negative_slope"].default == 0.2
    assert sig(ops.GatStack.train_step)[:5] == ["self", "X", "target", "rows", "lr"]
    for name in ("forward", "backward", "step", "grad_buffer", "train_step", "evaluate"):
        assert callable(getattr(ops.GatStack, name))
    assert "DIAG_FILL" in ops.GatStack.__doc__
    assert callable(ops.CsrGraph.attention_map)
