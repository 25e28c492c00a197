"""CPU checks behind tests/test_gpu_loss.py and tests/test_gpu_mask_calls.py (no device): the restatements of tests/loss_ref.py on
hand-written literals; every dyadic family really is exact (float32 evaluations in two orders and the int64 evaluation agree bit
for bit at the largest shapes the GPU tests use); every family tells a wrong result from the right one (a dropped last row, a
skipped last float4, a row counted twice, argmax with >=, a restriction that sorts); and what the loss entry points refuse before
they touch a device."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from tests import loss_ref as lr
from tests import sddmm_ref
from tests.helpers import pkg  # noqa: F401


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. literals
def test_softmax_ce_ref64_literals():
    X = np.array([[0.0, math.log(3.0)], [0.0, 0.0]])
    loss, d, cs, rl = lr.softmax_ce_ref64(X, [0, 1])
    assert abs(rl[0] - math.log(4.0)) <= 1e-15 and abs(rl[1] - math.log(2.0)) <= 1e-15
    assert abs(loss - (math.log(4.0) + math.log(2.0)) / 2) <= 1e-15
    assert np.allclose(d[0], [-0.375, 0.375], rtol=0, atol=1e-16) and np.allclose(d[1], [0.25, -0.25], rtol=0, atol=1e-16)
    assert np.allclose(cs, [-0.125, 0.125], rtol=0, atol=1e-16)
    loss, d, cs, rl = lr.softmax_ce_ref64(X, [-1, 1], rows=[1], n_total=4)        # an unlisted row: no gradient, its target unread
    assert d[0] is None and np.allclose(d[1], [0.125, -0.125], rtol=0, atol=1e-16) and np.allclose(cs, d[1])
    assert abs(loss - math.log(2.0) / 4) <= 1e-15 and rl.shape == (1,)
    # the + 1e-20 of the denominator is there: one class, x = -50, p = e / (e + 1e-20)
    loss, d, _, _ = lr.softmax_ce_ref64(np.array([[-50.0]]), [0])
    e = math.exp(-50.0)
    assert abs(loss - math.log1p(1e-20 / e)) <= 1e-12 and abs(d[0][0] - (e / (e + 1e-20) - 1.0)) <= 1e-15
    # no max-subtraction: exp overflows, the row is NaN
    loss, d, _, _ = lr.softmax_ce_ref64(np.array([[800.0, 0.0]]), [1])
    assert not np.isfinite(d[0][0]) and d[0][1] == -1.0                           # inf / inf; 1 / inf - 1
    # a fully dead row: -onehot / n_total and an infinite loss
    loss, d, _, rl = lr.softmax_ce_ref64(np.array([[-np.inf, -np.inf, -np.inf]]), [2], n_total=4)
    assert np.array_equal(d[0], [0.0, 0.0, -0.25]) and rl[0] == np.inf and loss == np.inf
    assert lr.bce_ref64 is sddmm_ref.bce_logits_ref64


def test_dyadic_literals():
    X = np.array([[0.0, -np.inf, 0.0, -np.inf], [-200.0, 0.0, -200.0, -200.0], [-200.0] * 4], dtype=np.float32)
    G, cs = lr.dyadic_ce_int(X, [0, 3, 1])
    assert G.tolist() == [[-4, 0, 4, 0], [0, 8, 0, -8], [0, -8, 0, 0]] and cs.tolist() == [-4, 0, 4, -8]
    assert lr.dyadic_to_f32(G, 4)[0].tolist() == [-0.125, 0.0, 0.125, 0.0]
    with pytest.raises(AssertionError):
        lr.dyadic_to_f32(G, 3)
    s, g = lr.bce_dyadic_int(np.array([128, -128, 256, 0], dtype=np.float32), np.array([0.25, 1, 0, 0.25], dtype=np.float32))
    assert s == 96 + 128 + 256 and g.tolist() == [0.75, -1.0, 1.0, 0.25]
    X, t = lr.heavy_row_case(3, 4, 1, -np.inf)
    assert t.tolist() == [0, 1, 2] and X[1].tolist() == [-np.inf, -64.0, 0.0, -np.inf] and X[0].tolist() == [0.0] + [-np.inf] * 3
    assert lr.edge_columns(260) == [0, 3, 4, 255, 256, 259] and lr.edge_columns(4) == [0, 3] and lr.edge_columns(1) == [0]


def test_mask_and_argmax_ref_literals():
    assert lr.mask_rows_ref(np.array([0, 2, 0, 0x80, 1, 0], dtype=np.uint8)).tolist() == [1, 3, 4]
    assert lr.mask_rows_ref(np.zeros(3, dtype=np.uint8)).shape == (0,)
    rp, ci, v = [0, 2, 2, 5], [2, 0, 1, 1, 0], np.array([10, 11, 12, 13, 14], dtype=np.float32)
    a = lr.restrict_ref(rp, ci, v, np.array([1, 1, 0], dtype=np.uint8), None)
    assert a[0].tolist() == [0, 2, 2, 2] and a[1].tolist() == [2, 0] and a[2].tolist() == [10, 11]
    a = lr.restrict_ref(rp, ci, v, None, np.array([0xFF, 0, 2], dtype=np.uint8))
    assert a[0].tolist() == [0, 2, 2, 3] and a[1].tolist() == [2, 0, 0] and a[2].tolist() == [10, 11, 14]
    a = lr.restrict_ref(rp, ci, None, np.array([0, 1, 1], dtype=np.uint8), np.array([0, 1, 0], dtype=np.uint8))
    assert a[0].tolist() == [0, 0, 0, 2] and a[1].tolist() == [1, 1] and a[2] is None
    a = lr.restrict_ref(rp, ci, v, None, None)
    assert a[0].tolist() == rp and a[1].tolist() == ci and a[2].tolist() == v.tolist()
    X = np.array([[-0.0, 0.0, 0.0], [-np.inf] * 3, [1.0, np.inf, np.inf], [-2.0, 1.0, 1.0], [-np.inf, -1.0, -2.0]], dtype=np.float32)
    assert lr.argmax_first_ref(X).tolist() == [0, 0, 1, 1, 1]
    with pytest.raises(ValueError):
        lr.argmax_first_ref(np.array([[0.0, np.nan]], dtype=np.float32))


# ------------------------------------------------------------------ 2. the dyadic families are exact
CE_LARGEST = [(32769, 5, 1 << 16), (16385, 4, 1 << 15), (513, 1032, 1 << 10), (17, 1028, 32), (17, 1024, 32), (16385, 260, 1 << 15)]


def family(name, n, C, dead):
    if name == "dense":
        return lr.dense(5, n, C, dead)
    if name == "edges":
        return lr.edges(n, C, dead)
    return lr.target_dead(7, n, C, dead)


@pytest.mark.parametrize("name", ["dense", "edges", "target_dead"])
@pytest.mark.parametrize("n,c,n_total", CE_LARGEST)
def test_ce_dyadic_families_are_exact_in_every_order(name, n, c, n_total):
    dead = lr.DEAD_VALUES[(n + c) % 2]
    X, t = family(name, n, c, dead)
    G, cs = lr.dyadic_ce_int(X, t)
    want_d, want_cs = lr.dyadic_to_f32(G, n_total), lr.dyadic_to_f32(cs, n_total)
    rng = np.random.default_rng(1)
    d1, cs1 = lr.softmax_ce_f32(X, t, n_total)
    d2, cs2 = lr.softmax_ce_f32(X, t, n_total, class_order=range(c - 1, -1, -1), row_order=rng.permutation(n))
    for d, s in ((d1, cs1), (d2, cs2)):
        assert np.array_equal(bits(d), bits(want_d)) and np.array_equal(bits(s), bits(want_cs))
    # and float64 says the same (there exp(-200) is 1e-87, not 0: equal once rounded to f32)
    _, d64, cs64, rl = lr.softmax_ce_ref64(X[:40], t[:40], n_total=n_total)
    assert np.array_equal(bits(np.stack(d64).astype(np.float32)), bits(want_d[:40]))
    if name == "target_dead":
        assert np.all(rl == np.inf) if dead == -np.inf else np.all(rl > 100.0)     # (float64; in f32 exp(-200) = 0 and the row loss is +inf either way)
    else:
        assert np.all(np.isfinite(rl))


@pytest.mark.parametrize("n", [1, 65537, 131073])
def test_bce_dyadic_family_is_exact_in_every_order(n):
    x, y = lr.bce_dyadic(3, n)
    total, g = lr.bce_dyadic_int(x, y)
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(x))
    assert e.dtype == np.float32 and not e.any()
    terms = (np.maximum(x, np.float32(0)) - x * y) + np.log1p(e)
    assert terms.dtype == np.float32
    fwd, rev, pair = np.cumsum(terms, dtype=np.float32)[-1], np.cumsum(terms[::-1], dtype=np.float32)[-1], terms.sum(dtype=np.float32)
    assert float(fwd) == float(rev) == float(pair) == float(total)
    n_total = 1 << 18
    assert np.float32(total) * (np.float32(1) / np.float32(n_total)) == total / n_total
    sig = np.where(x >= 0, np.float32(1) / (np.float32(1) + e), e / (np.float32(1) + e))
    d = (sig - y) * (np.float32(1) / np.float32(n_total))
    assert np.array_equal(d.astype(np.float64), g / n_total)
    xz, yz = lr.bce_dyadic(3, 1000, with_zero=True)
    assert (xz == 0).any()
    _, gz = lr.bce_dyadic_int(xz, yz)
    assert np.array_equal(bits(gz), bits(sddmm_ref.bce_logits_ref64(xz, yz)[1]))     # float64's sigmoid(-128) = 3e-56 is 0 in f32


# ------------------------------------------------------------------ 3. each family tells wrong from right
VEC_C = (4, 252, 256, 260, 512, 516, 768, 772, 1020, 1024)


@pytest.mark.parametrize("name", ["dense", "edges", "target_dead"])
def test_a_dropped_last_row_changes_the_column_sums(name):
    for n, c in ((2, 4), (17, 5), (16385, 4), (513, 1032)):
        X, t = family(name, n, c, -np.inf)
        G, cs = lr.dyadic_ce_int(X, t)
        assert G[-1].any() and not np.array_equal(cs - G[-1], cs)
        assert G[0].any()


@pytest.mark.parametrize("c", VEC_C)
def test_a_skipped_last_float4_changes_the_column_sums_of_the_edges_family(c):
    X, t = lr.edges(17, c, -200.0)
    G, cs = lr.dyadic_ce_int(X, t)
    cols = lr.edge_columns(c)
    assert all(np.abs(G[:, col]).sum() > 0 for col in cols)            # every edge column carries mass
    assert cs[c - 4:].any(), "the last float4 sums to zero: a kernel that skips it would pass the column sums"
    assert G[:, c - 4:].any(1).sum() >= 8


def test_a_row_counted_twice_moves_the_heavy_row_loss():
    X, t = lr.heavy_row_case(9, 4, 8, -np.inf)
    loss, _, _, rl = lr.softmax_ce_ref64(X, t, n_total=16)
    assert np.count_nonzero(rl) == 1 and abs(rl[8] - 64.0) < 1e-6 and loss == rl[8] / 16
    ulp = np.spacing(np.float32(loss))
    assert abs(2 * loss - loss) > 8 * ulp and abs(0.0 - loss) > 8 * ulp          # twice, or not at all
    G, cs = lr.dyadic_ce_int(*lr.dense(5, 9, 4, -np.inf))
    assert not np.array_equal(cs + G[3], cs) or not G[3].any()


@pytest.mark.parametrize("c", [2, 63, 64, 65, 127, 128, 129, 1000])
def test_argmax_with_ge_differs_on_the_tie_inputs(c):
    X = lr.argmax_case(c, 5, c)
    ref = lr.argmax_first_ref(X)
    last = np.array([max(range(c), key=lambda j: (row[j], j)) for row in X.tolist()])      # >= keeps the LAST maximum
    assert np.array_equal(ref, np.argmax(X, 1))
    assert (last != ref).any()
    # "lower index wins" reversed in the butterfly alone (lanes c % 64): visible once two lanes tie
    assert ((X == X.max(1, keepdims=True)).sum(1) > 1).any()


def test_a_sorting_restriction_differs_on_unsorted_dups():
    n, nc, rp, ci = lr.tiny_csr_patterns()["unsorted_dups"]
    keep = np.ones(nc, dtype=np.uint8)
    keep[5] = 0
    _, got, _ = lr.restrict_ref(rp, ci, None, None, keep)
    rp2, _, _ = lr.restrict_ref(rp, ci, None, None, keep)
    sorted_rows = np.concatenate([np.sort(got[rp2[r]:rp2[r + 1]]) for r in range(n)])
    assert not np.array_equal(sorted_rows, got)
    P = lr.tiny_csr_patterns()
    assert sorted(P) == sorted(["empty", "one_entry", "lead_trail_empty", "row64", "row65", "row128", "straddle", "many_empty", "rect",
                                "unsorted_dups", "one_row"])
    for name, (n, nc, rp, ci) in P.items():
        assert len(rp) == n + 1 and rp[-1] == len(ci) and (len(ci) == 0 or (0 <= ci.min() and ci.max() < nc)), name
    assert P["empty"][2].tolist() == [0, 0, 0, 0] and len(P["row64"][3]) == 64 and len(P["row65"][3]) == 65 and len(P["row128"][3]) == 128
    assert P["rect"][0] == 5 and P["rect"][1] == 300 and P["one_row"][0] == 1 and len(P["one_row"][3]) == 130
    assert P["lead_trail_empty"][2][:3].tolist() == [0, 0, 0] and np.all(P["lead_trail_empty"][2][-3:] == P["lead_trail_empty"][2][-1])


# ------------------------------------------------------------------ 4. refusals that need no device
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_softmax_ce_refusals_without_device(capi):
    """Every refusal returns before a device call: the pointers are HOST arrays holding sentinels, unchanged afterwards."""
    L = capi.lib()
    n, c = 6, 8
    X, t, rows = np.full((n, c), 3.0, dtype=np.float32), np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    loss, d, cs = np.full(1, 7.0, dtype=np.float32), np.full((n, c), 7.0, dtype=np.float32), np.full(c, 7.0, dtype=np.float32)
    need = C.c_size_t(0)
    assert L.gnnx_softmax_ce_colsum_workspace(n, c, C.byref(need)) == 0
    ws = np.full(need.value + 512, 0x5A, dtype=np.uint8)

    def partial(n_rows=n, n_classes=c, n_total=n, ldx=c, ldd=c, dl=d, cs_=cs, w=ws, bytes_=None):
        return L.gnnx_softmax_ce_partial_f32(ptr(X), ldx, ptr(t), n_rows, n_classes, n_total, ptr(loss), None if dl is None else ptr(dl), ldd,
                                             None if cs_ is None else ptr(cs_), None if w is None else ptr(w),
                                             need.value if bytes_ is None else bytes_, None)

    def listed(n_listed=n, n_rows=n, n_classes=c, n_total=n, ldx=c, ldd=c, dl=d, cs_=cs, w=ws, bytes_=None):
        return L.gnnx_softmax_ce_rows_f32(ptr(X), ldx, ptr(t), ptr(rows), n_listed, n_rows, n_classes, n_total, ptr(loss),
                                          None if dl is None else ptr(dl), ldd, None if cs_ is None else ptr(cs_),
                                          None if w is None else ptr(w), need.value if bytes_ is None else bytes_, None)

    for call in (partial, listed):
        assert call(n_total=n - 1) == -1 and "n_total" in L.gnnx_last_error().decode()
        assert call(ldx=c - 1) == -1
        assert call(ldd=c - 1) == -1 and "ldd" in L.gnnx_last_error().decode()
        assert call(dl=None) == -1 and "column sums" in L.gnnx_last_error().decode()
        assert call(n_classes=0) == -1
        assert call(w=None) == -4
        assert call(bytes_=need.value - 1) == -4
    assert listed(n_rows=n - 1) == -1 and "more listed rows" in L.gnnx_last_error().decode()
    assert listed(n_listed=0) == -1
    # ldd < C without a gradient is not an error of its own: the call goes on to the next check (a short workspace here)
    assert partial(ldd=0, dl=None, cs_=None, bytes_=0) == -4
    # the plain and the column-sum entry points share the driver
    assert L.gnnx_softmax_ce_colsum_f32(ptr(X), c - 1, ptr(t), n, c, ptr(loss), ptr(d), c, ptr(cs), ptr(ws), need.value, None) == -1
    assert L.gnnx_softmax_ce_colsum_f32(ptr(X), c, ptr(t), n, c, ptr(loss), None, c, ptr(cs), ptr(ws), need.value, None) == -1
    assert L.gnnx_softmax_ce_colsum_f32(ptr(X), c, ptr(t), n, c, ptr(loss), ptr(d), c, ptr(cs), ptr(ws), need.value - 1, None) == -4
    small = C.c_size_t(0)
    assert L.gnnx_softmax_ce_workspace(n, C.byref(small)) == 0
    assert L.gnnx_softmax_ce_f32(ptr(X), c, ptr(t), n, c, ptr(loss), ptr(d), c - 1, ptr(ws), small.value, None) == -1
    assert L.gnnx_softmax_ce_f32(ptr(X), c, ptr(t), n, c, ptr(loss), ptr(d), c, None, small.value, None) == -4
    assert L.gnnx_softmax_ce_f32(ptr(X), c, ptr(t), n, c, ptr(loss), ptr(d), c, ptr(ws), small.value - 1, None) == -4
    assert L.gnnx_softmax_ce_f32(ptr(X), c, ptr(t), n, 0, ptr(loss), ptr(d), c, ptr(ws), small.value, None) == -1
    assert loss[0] == 7.0 and np.all(d == 7.0) and np.all(cs == 7.0) and np.all(ws == 0x5A) and np.all(X == 3.0)


def test_bce_refusals_without_device(capi):
    L = capi.lib()
    n = 5
    x, y = np.full(n, 2.0, dtype=np.float32), np.full(n, 1.0, dtype=np.float32)
    loss, d = np.full(1, 7.0, dtype=np.float32), np.full(n, 7.0, dtype=np.float32)
    need = C.c_size_t(0)
    assert L.gnnx_bce_logits_workspace(n, C.byref(need)) == 0 and need.value > 0
    ws = np.full(need.value, 0x5A, dtype=np.uint8)
    bce = L.gnnx_bce_logits_f32
    assert bce(ptr(x), ptr(y), n, n - 1, ptr(loss), ptr(d), ptr(ws), need.value, None) == -1 and "n_total" in L.gnnx_last_error().decode()
    assert bce(ptr(x), ptr(y), n, n, ptr(loss), ptr(d), ptr(ws), need.value - 1, None) == -4
    assert bce(ptr(x), ptr(y), n, n, ptr(loss), None, None, need.value, None) == -4
    assert bce(ptr(x), ptr(y), n, n, None, None, None, 0, None) == 0                  # nothing asked for: nothing done
    assert loss[0] == 7.0 and np.all(d == 7.0) and np.all(ws == 0x5A)


def test_loss_workspace_queries(capi):
    L = capi.lib()
    a, b, p = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    prev = {}
    for c in (1, 4, 5, 256, 1000, 1032):
        prev[c] = 0
        for n in (0, 1, 7, 8, 9, 255, 256, 257, 16383, 16384, 16385, 65537, 1 << 20):
            assert L.gnnx_softmax_ce_rows_workspace(n, c, C.byref(a)) == 0 and L.gnnx_softmax_ce_colsum_workspace(n, c, C.byref(b)) == 0
            assert L.gnnx_softmax_ce_workspace(n, C.byref(p)) == 0
            assert a.value == b.value and 0 < p.value <= b.value
            assert b.value >= prev[c], (n, c)
            prev[c] = b.value
    last = 0
    for n in (0, 1, 9, 16385, 65537, 1 << 20):
        assert L.gnnx_softmax_ce_workspace(n, C.byref(p)) == 0 and p.value >= last
        last = p.value
    assert L.gnnx_bce_logits_workspace(1, C.byref(a)) == 0 and L.gnnx_bce_logits_workspace(1 << 20, C.byref(b)) == 0 and a.value <= b.value
