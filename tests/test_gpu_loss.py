"""GPU tests of the loss kernels of gnnx_train.hip (run with -m gpu on an MI355X): every form of the softmax cross-entropy (vector
form KV = 1..4, generic walk, generic column-sum pass, plain / shard / listed entry points) and the binary cross-entropy, each path
and edge against tests/loss_ref.py.  tests/test_gpu_parity.py and tests/test_gpu_masked.py hold the workload shapes.

Bars
  * DYADIC inputs (tests/loss_ref.py: logits 0 or dead, k in {0, 1, 2, 4, 8} zeros per row, n_total = 2^b): nothing rounds on any
    path, so dlogits and the column sums must have the BITS of the int64 evaluation, whatever the summation order.
  * general data (synth.uniform_pm1 * 3, and amplitude 20), per element against float64, p = softmax, d = onehot:
        gradient     |d - (p - d) / n_total| <= (S + 8) * 2^-24 * (p + d) / n_total
        column sums  |cs - ref|              <= (S + 8 + n_listed) * 2^-24 * sum_i (p + d) / n_total           (sequential worst case)
        loss         |loss - ref|            <= 2^-24 * [(S + 4) n_listed + (ceil(n_listed / 65536) + 266) sum |l_i|] / n_total
    S = additions on the path of a row sum: 4 ceil(C / 256) + 6 on the vector form, ceil(C / 64) + 6 on the generic walk.  The 8:
    expf on the element and on the sum, + 1e-20, the reciprocal, the product, the subtraction, 1 / n_total and the product with it.
    Derived, not measured; the worst observed ratio error / (2^-24 * scale) per form is printed when the module finishes.
    The amplitude-20 case is uniform_pm1 * 20, not 3 * 20: with logits in +-60 a probability goes down to e^-120 = 8e-53, below the
    smallest f32 number, where no relative bound can hold; +-20 gives p >= e^-40 = 4e-18 and p / n_total stays a normal number.
  * heavy-row loss: one row with l = 64, every other row exactly 0: loss within 8 ulp of l / n_total iff the row counts once.
  * BCE: dyadic inputs bit-exact against integers; general data per element |d - ref| <= 6 * 2^-24 * (sigmoid + y) / n_total and
    |loss - ref| <= 2^-24 * (9 + ceil(n / 65536) + 266) * sum_p a_p / n_total, a_p = max(x, 0) + |x y| + log1p(exp(-|x|)) (9: the
    product, the subtraction, the addition, expf and log1pf at 1.5 ulp each; the rest is the depth of the sum, as for the loss above).
    The special scores -88 and -100 carry y > 0 here: sigmoid(-100) = 4e-44 is a denormal, which no relative bound fits.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import loss_ref as lr
from tests.helpers import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
VEC_C = (4, 252, 256, 260, 512, 516, 768, 772, 1020, 1024)
GEN_C = (1, 2, 3, 5, 63, 64, 65, 127, 129, 1028, 1032)
SMALL_N = (1, 2, 7, 8, 9, 15, 17)
NAN_BITS = 0x7FC00000
RATIOS = {}          # (form, quantity) -> (worst observed ratio, its bound there)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    yield dict(torch=torch, capi=capi, L=capi.lib(), dev=torch.device("cuda:0"))
    for (form, what), (ratio, bound) in sorted(RATIOS.items()):
        print(f"worst ratio  {form:8s} {what:8s} {ratio:10.3f}  (bound {bound:.1f})")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pow2_at_least(n):
    return 1 << max(0, int(n - 1).bit_length())


def is_vec(c, ldx, ldd, x_off, d_off, grad):
    return c % 4 == 0 and c <= 1024 and ldx % 4 == 0 and x_off % 4 == 0 and (not grad or (ldd % 4 == 0 and d_off % 4 == 0))


def adds(c, vec):
    return 4 * -(-c // 256) + 6 if vec else -(-c // 64) + 6


# ------------------------------------------------------------------ the harness
def run_ce(env, X, t, call="partial", rows=None, n_total=None, loss=True, grad=True, colsum=True, ldx=None, x_off=0, ldd=None, d_off=0,
           ws_off=0):
    """One call of gnnx_softmax_ce_{f32 (plain), colsum_f32 (colsum), partial_f32 (partial), rows_f32 (rows)} on poisoned buffers.
    Logits and gradient live at float offset x_off / d_off of NaN-filled buffers with row strides ldx / ldd; the workspace is the
    queried size exactly, at byte offset ws_off of a 0xFF-filled buffer with 64 guard bytes behind.  Everything the call must not
    touch is checked here; returns (status, dict of host arrays)."""
    torch, L, dv = env["torch"], env["L"], env["dev"]
    n, c = X.shape
    ldx, ldd = ldx or c, ldd or c
    nl = n if rows is None else len(rows)
    n_total = nl if n_total is None else n_total
    xbuf = torch.full((x_off + n * ldx,), float("nan"), dtype=torch.float32, device=dv)
    xbuf[x_off:].view(n, ldx)[:, :c] = torch.from_numpy(np.ascontiguousarray(X)).to(dv)
    x_before = xbuf.view(torch.int32).clone()
    gbuf = torch.full((d_off + n * ldd,), float("nan"), dtype=torch.float32, device=dv)
    lbuf = torch.full((3,), float("nan"), dtype=torch.float32, device=dv)
    cbuf = torch.full((c + 2,), float("nan"), dtype=torch.float32, device=dv)
    td = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(dv)
    rd = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dv)
    assert xbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    need = C.c_size_t(0)
    if call == "plain":
        assert not colsum and rows is None and n_total == n
        assert L.gnnx_softmax_ce_workspace(n, C.byref(need)) == 0
    elif call == "rows":
        assert L.gnnx_softmax_ce_rows_workspace(nl, c, C.byref(need)) == 0
    else:
        assert L.gnnx_softmax_ce_colsum_workspace(n, c, C.byref(need)) == 0
    ws = torch.full((ws_off + need.value + 64,), 0xFF, dtype=torch.uint8, device=dv)
    px, pg = xbuf.data_ptr() + 4 * x_off, (gbuf.data_ptr() + 4 * d_off) if grad else None
    pl, pc, pw = (lbuf.data_ptr() + 4) if loss else None, (cbuf.data_ptr() + 4) if colsum else None, ws.data_ptr() + ws_off
    if call == "plain":
        st = L.gnnx_softmax_ce_f32(px, ldx, td.data_ptr(), n, c, pl, pg, ldd, pw, need.value, None)
    elif call == "colsum":
        assert rows is None and n_total == n
        st = L.gnnx_softmax_ce_colsum_f32(px, ldx, td.data_ptr(), n, c, pl, pg, ldd, pc, pw, need.value, None)
    elif call == "partial":
        assert rows is None
        st = L.gnnx_softmax_ce_partial_f32(px, ldx, td.data_ptr(), n, c, n_total, pl, pg, ldd, pc, pw, need.value, None)
    else:
        st = L.gnnx_softmax_ce_rows_f32(px, ldx, td.data_ptr(), rd.data_ptr(), nl, n, c, n_total, pl, pg, ldd, pc, pw, need.value, None)
    torch.cuda.synchronize()
    assert torch.equal(xbuf.view(torch.int32), x_before), "the logits buffer changed"
    wsh = ws.cpu().numpy()
    assert np.all(wsh[:ws_off] == 0xFF) and np.all(wsh[ws_off + need.value:] == 0xFF), "bytes outside the queried workspace changed"
    gh, lh, ch = gbuf.cpu().numpy(), lbuf.cpu().numpy(), cbuf.cpu().numpy()
    assert np.all(bits(gh[:d_off]) == NAN_BITS), "floats in front of the gradient base changed"
    Gfull = gh[d_off:].reshape(n, ldd)
    assert np.all(bits(Gfull[:, c:]) == NAN_BITS), "pad columns of the gradient changed"
    assert bits(lh)[0] == NAN_BITS and bits(lh)[2] == NAN_BITS and bits(ch)[0] == NAN_BITS and bits(ch)[-1] == NAN_BITS
    if not loss:
        assert bits(lh)[1] == NAN_BITS
    if not colsum:
        assert np.all(bits(ch) == NAN_BITS)
    if not grad:
        assert np.all(bits(gh) == NAN_BITS)
    return st, dict(loss=lh[1:2].copy(), G=np.ascontiguousarray(Gfull[:, :c]), cs=ch[1:-1].copy())


def note(form, what, ratio, bound):
    if ratio > RATIOS.get((form, what), (-1.0, 0.0))[0]:
        RATIOS[(form, what)] = (ratio, bound)


def check_general(out, X, t, rows, n_total, vec, what, loss=True, grad=True, colsum=True):
    """The three per-element bounds of the module docstring against softmax_ce_ref64; unlisted gradient rows keep the sentinel."""
    n, c = X.shape
    sel = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    nl = len(sel)
    loss_ref, d_ref, cs_ref, rl = lr.softmax_ce_ref64(X, t, rows, n_total)
    P = lr.softmax_probs64(X, sel)
    scale = P.copy()
    scale[np.arange(nl), np.asarray(t)[sel]] += 1.0                 # p + onehot
    S, form = adds(c, vec), "vector" if vec else "generic"
    if grad:
        err = np.abs(out["G"][sel].astype(np.float64) - np.stack([d_ref[r] for r in sel]))
        assert not err[scale == 0].any(), f"{what}: a class of probability 0 off the target has a non-zero gradient"
        ratio = float((err[scale > 0] / (U * scale[scale > 0] / n_total)).max())
        note(form, "gradient", ratio, S + 8)
        print(f"{what}: gradient ratio {ratio:.3f} bound {S + 8}")
        assert ratio <= S + 8, f"{what}: gradient error / (2^-24 (p + onehot) / n_total) = {ratio:.3f} > {S + 8}"
        others = np.ones(n, dtype=bool)
        others[sel] = False
        assert np.all(bits(out["G"][others]) == NAN_BITS), f"{what}: an unlisted gradient row was written"
    if colsum:
        err = np.abs(out["cs"].astype(np.float64) - cs_ref)
        ratio = float((err / (U * scale.sum(0) / n_total)).max())
        note(form, "colsum", ratio, S + 8 + nl)
        print(f"{what}: column-sum ratio {ratio:.3f} bound {S + 8 + nl}")
        assert ratio <= S + 8 + nl, f"{what}: column-sum error ratio {ratio:.3f} > {S + 8 + nl}"
    if loss:
        depth = -(-nl // 65536) + 8 + 256 + 2
        bound = U * ((S + 4) * nl + depth * np.abs(rl).sum()) / n_total
        err = abs(float(out["loss"][0]) - loss_ref)
        note(form, "loss", err / bound, 1.0)
        if np.abs(rl).sum() >= nl:                                      # (C = 1: every row loss is about 0, no scale to relate to)
            note(form, "loss/sum", err / (U * np.abs(rl).sum() / n_total), (S + 4) * nl / np.abs(rl).sum() + depth)
        print(f"{what}: loss {out['loss'][0]:.9g} ref {loss_ref:.9g} error / bound {err / bound:.4f}")
        assert err <= bound, f"{what}: loss error {err:.3e} > {bound:.3e}"


def check_dyadic(out, X, t, rows, n_total, what, colsum=True):
    n, c = X.shape
    sel = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    G, cs = lr.dyadic_ce_int(X, t, rows)
    assert np.array_equal(bits(out["G"][sel]), bits(lr.dyadic_to_f32(G, n_total))), f"{what}: gradient bits"
    others = np.ones(n, dtype=bool)
    others[sel] = False
    assert np.all(bits(out["G"][others]) == NAN_BITS), f"{what}: an unlisted gradient row was written"
    if colsum:
        assert np.array_equal(bits(out["cs"]), bits(lr.dyadic_to_f32(cs, n_total))), f"{what}: column-sum bits"


def family(name, n, c, dead):
    if name == "dense":
        return lr.dense(100 + n + c, n, c, dead)
    if name == "edges":
        return lr.edges(n, c, dead)
    return lr.target_dead(200 + n + c, n, c, dead)


def general(seed, n, c, amplitude=3.0):
    return synth.uniform_pm1(seed, (n, c)) * np.float32(amplitude), ((7 * np.arange(n) + 3) % c).astype(np.int32)


# ------------------------------------------------------------------ 1. every class count, small row counts
@pytest.mark.parametrize("name", ["dense", "edges", "target_dead"])
@pytest.mark.parametrize("c", VEC_C + GEN_C)
def test_ce_dyadic_class_counts(env, c, name):
    for n in SMALL_N:
        dead = lr.DEAD_VALUES[(n + c) % 2]
        X, t = family(name, n, c, dead)
        n_total = 4 * pow2_at_least(n)
        what = f"{name} n={n} C={c} dead={dead}"
        st, a = run_ce(env, X, t, "partial", n_total=n_total)
        assert st == 0
        check_dyadic(a, X, t, None, n_total, what)
        st, b = run_ce(env, X, t, "rows", rows=np.arange(n), n_total=n_total)
        assert st == 0
        assert same_bits(a["G"], b["G"]) and same_bits(a["cs"], b["cs"]) and same_bits(a["loss"], b["loss"]), what
        # gnnx_softmax_ce_colsum_f32 divides by n itself: one more rounding per element when n is no power of two
        st, d = run_ce(env, X, t, "colsum")
        assert st == 0
        G, cs = lr.dyadic_ce_int(X, t)
        assert np.array_equal(bits(d["G"]), bits(lr.dyadic_to_f32(G, 1) * (np.float32(1.0) / np.float32(n)))), what
        if n == pow2_at_least(n):
            assert np.array_equal(bits(d["cs"]), bits(lr.dyadic_to_f32(cs, n))), what
        if name == "target_dead":
            assert not np.isfinite(a["loss"][0]) and not np.isfinite(d["loss"][0]), what       # +inf: the target's exp is 0
        else:
            assert np.isfinite(a["loss"][0]), what
            k = (X == 0).sum(1)
            ref = np.log(k.astype(np.float64)).sum() / n_total                                # row loss = log k
            assert abs(float(a["loss"][0]) - ref) <= U * ((adds(c, c in VEC_C) + 4) * n + 267 * ref * n_total) / n_total, what


@pytest.mark.parametrize("c", VEC_C + GEN_C)
def test_ce_general_class_counts(env, c):
    vec = c in VEC_C
    for n in SMALL_N:
        X, t = general(900 + c, n, c)
        st, a = run_ce(env, X, t, "colsum")
        assert st == 0
        check_general(a, X, t, None, n, vec, f"colsum n={n} C={c}")
        st, b = run_ce(env, X, t, "rows", rows=np.arange(n), n_total=2 * n + 1)
        assert st == 0
        check_general(b, X, t, np.arange(n), 2 * n + 1, vec, f"rows n={n} C={c}")
    X, t = general(950 + c, 9, c, amplitude=20.0)           # probabilities from e^-40 to 1
    st, a = run_ce(env, X, t, "colsum")
    assert st == 0
    check_general(a, X, t, None, 9, vec, f"amplitude 20, n=9 C={c}")


# ------------------------------------------------------------------ 2. row seams
@pytest.mark.parametrize("n", [16383, 16384, 16385, 32769])
@pytest.mark.parametrize("c", [4, 5])
def test_ce_row_seams(env, n, c):
    """Vector grid: 2048 groups x 4 waves x 2 rows in flight = 16384 rows a sweep (the tail with one row in flight, the second sweep);
    the generic kernel has a wave per row, and its column-sum pass 256 blocks of ceil(n / 256) rows."""
    X, t = lr.dense(300 + n, n, c, lr.DEAD_VALUES[n % 2])
    n_total = 1 << 16
    st, a = run_ce(env, X, t, "partial", n_total=n_total)
    assert st == 0
    check_dyadic(a, X, t, None, n_total, f"seam n={n} C={c}")
    st, b = run_ce(env, X, t, "rows", rows=np.arange(n), n_total=n_total)
    assert st == 0 and same_bits(a["G"], b["G"]) and same_bits(a["cs"], b["cs"]) and same_bits(a["loss"], b["loss"])
    k = (X == 0).sum(1)
    ref = np.log(k.astype(np.float64)).sum() / n_total
    assert abs(float(a["loss"][0]) - ref) <= U * ((adds(c, c == 4) + 4) * n + 267 * ref * n_total) / n_total


@pytest.mark.parametrize("n", [255, 256, 257, 511, 513])
@pytest.mark.parametrize("c", [5, 1032])
def test_ce_generic_column_sum_seams(env, n, c):
    """ce_colsum_generic: min(n, 256) blocks of ceil(n / 256) rows -- one row a block up to 256, then two with a ragged last block."""
    X, t = lr.dense(400 + n, n, c, lr.DEAD_VALUES[n % 2])
    st, a = run_ce(env, X, t, "partial", n_total=1024)
    assert st == 0
    check_dyadic(a, X, t, None, 1024, f"dyadic n={n} C={c}")
    X, t = general(410 + n, n, c)
    st, a = run_ce(env, X, t, "colsum")
    assert st == 0
    check_general(a, X, t, None, n, False, f"general n={n} C={c}")


# ------------------------------------------------------------------ 3. the heavy row: counted exactly once
@pytest.mark.parametrize("n", [9, 16385, 65537])
def test_ce_heavy_row_is_counted_once(env, n):
    """sum_stage1 sweeps 65536 elements, the vector grid 16384 rows: a heavy row on each side of every seam."""
    c, n_total = 4, pow2_at_least(n)
    for r in sorted({r for r in (0, 7, 8, 8191, 8192, 16383, 16384, 65535, 65536, n - 1) if r < n}):
        X, t = lr.heavy_row_case(n, c, r, lr.DEAD_VALUES[r % 2])
        ref = lr.softmax_ce_ref64(X[r:r + 1], t[r:r + 1])[3][0] / n_total
        for call, rows in (("partial", None), ("rows", np.arange(n))):
            st, a = run_ce(env, X, t, call, rows=rows, n_total=n_total, grad=False, colsum=False)
            got = float(a["loss"][0])
            print(f"n={n} heavy row {r} {call}: loss {got:.9g} ref {ref:.9g} ({abs(got - ref) / np.spacing(np.float32(ref)):.2f} ulp)")
            assert st == 0 and abs(got - ref) <= 8 * np.spacing(np.float32(ref)), (n, r, call, got, ref)


# ------------------------------------------------------------------ 4. leaving the vector form, one condition at a time
LEAVE = [dict(ldx=1), dict(ldx=4, x_off=1), dict(ldd=1), dict(ldd=4, d_off=1)]


@pytest.mark.parametrize("c", [256, 1024])
@pytest.mark.parametrize("how", LEAVE, ids=["ldx", "logits-base", "ldd", "gradient-base"])
def test_ce_leaves_the_vector_form(env, c, how):
    """Each of ldx % 4, aligned16(logits), ldd % 4, aligned16(dlogits) fails alone: the generic walk takes the call.  (run_ce holds the
    pad columns, the floats in front of the bases and the logits buffer to their NaN sentinels.)"""
    n = 9
    kw = dict(ldx=c + how.get("ldx", 0), ldd=c + how.get("ldd", 0), x_off=how.get("x_off", 0), d_off=how.get("d_off", 0))
    assert not is_vec(c, kw["ldx"], kw["ldd"], kw["x_off"], kw["d_off"], True) and is_vec(c, c, c, 0, 0, True)
    for name in ("dense", "edges", "target_dead"):
        X, t = family(name, n, c, lr.DEAD_VALUES[len(name) % 2])
        st, a = run_ce(env, X, t, "partial", n_total=16)
        st2, b = run_ce(env, X, t, "partial", n_total=16, **kw)
        assert st == 0 and st2 == 0
        check_dyadic(b, X, t, None, 16, f"{name} C={c} {how}")
        assert same_bits(a["G"], b["G"]) and same_bits(a["cs"], b["cs"])
    X, t = general(500 + c, n, c)
    for call, rows in (("colsum", None), ("rows", np.arange(0, n, 2))):
        st, b = run_ce(env, X, t, call, rows=rows, **kw)
        assert st == 0
        check_general(b, X, t, rows, n if rows is None else len(rows), False, f"general C={c} {how} {call}")
    # without a gradient the gradient's stride and base do not matter: the vector form again, the loss bits of the aligned call
    if "ldd" in how:
        st, a = run_ce(env, X, t, "partial", n_total=n, grad=False, colsum=False)
        st2, b = run_ce(env, X, t, "partial", n_total=n, grad=False, colsum=False, **kw)
        assert st == 0 and st2 == 0 and same_bits(a["loss"], b["loss"])


# ------------------------------------------------------------------ 5. listed rows
def row_lists(n):
    rng = np.random.default_rng(n)
    return {"first": np.array([0]), "last": np.array([n - 1]), "every-second": np.arange(0, n, 2),
            "one-percent": np.sort(rng.permutation(n)[:max(1, n // 100)]), "all": np.arange(n)}


@pytest.mark.parametrize("c", [5, 256])
def test_ce_listed_rows(env, c):
    n, vec = 300, c == 256
    Xd, td_ = lr.dense(600 + c, n, c, -np.inf)
    Xg, tg = general(610 + c, n, c)
    for lname, rows in row_lists(n).items():
        nl = len(rows)
        off = np.ones(n, dtype=bool)
        off[rows] = False
        t = np.where(off, -1, td_).astype(np.int32)                      # targets are -1 off the list
        n_total = pow2_at_least(nl)
        st, a = run_ce(env, Xd, t, "rows", rows=rows, n_total=n_total)
        assert st == 0
        check_dyadic(a, Xd, t, rows, n_total, f"listed {lname} C={c}")
        t = np.where(off, -1, tg).astype(np.int32)
        st, a = run_ce(env, Xg, t, "rows", rows=rows, n_total=2 * nl + 1)
        assert st == 0
        check_general(a, Xg, t, rows, 2 * nl + 1, vec, f"listed {lname} C={c}")
        if lname == "all":                                               # the bits of the plain call
            st, b = run_ce(env, Xg, tg, "partial", n_total=2 * nl + 1)
            assert st == 0 and same_bits(a["G"], b["G"]) and same_bits(a["cs"], b["cs"]) and same_bits(a["loss"], b["loss"])
    rows = np.arange(0, n, 2)
    for bad_row in (-1, n):
        for where in (0, len(rows) - 1):
            r = rows.copy()
            r[where] = bad_row
            assert run_ce(env, Xg, tg, "rows", rows=r)[0] == -3, (bad_row, where)
    for bad_t in (-1, c):
        for where in (rows[0], rows[-1]):
            t = tg.copy()
            t[where] = bad_t
            assert run_ce(env, Xg, t, "rows", rows=rows)[0] == -3, (bad_t, where)
            assert run_ce(env, Xg[::2], t[::2], "colsum")[0] == -3
    t = tg.copy()
    t[1] = c                                                             # a bad target at an unlisted row is never read
    assert run_ce(env, Xg, t, "rows", rows=rows)[0] == 0


# ------------------------------------------------------------------ 6. optional outputs, workspace placement
@pytest.mark.parametrize("c", [5, 256])
def test_ce_optional_outputs(env, c):
    """d_loss == NULL, d_dlogits == NULL, no column sums: what is written has the bits of the full call, and (run_ce) what is not
    asked for keeps its sentinel."""
    n = 9
    X, t = general(700 + c, n, c)
    rows = np.arange(0, n, 2)
    for call, r in (("partial", None), ("rows", rows)):
        st, full = run_ce(env, X, t, call, rows=r)
        assert st == 0
        for loss, grad, colsum in ((False, True, True), (True, False, False), (True, True, False), (False, True, False)):
            st, a = run_ce(env, X, t, call, rows=r, loss=loss, grad=grad, colsum=colsum)
            assert st == 0
            assert not loss or same_bits(a["loss"], full["loss"])
            assert not grad or same_bits(a["G"], full["G"])
            assert not colsum or same_bits(a["cs"], full["cs"])
    st, full = run_ce(env, X, t, "colsum")
    st2, a = run_ce(env, X, t, "plain", colsum=False)
    st3, b = run_ce(env, X, t, "plain", colsum=False, loss=False)
    st4, d = run_ce(env, X, t, "plain", colsum=False, grad=False)
    assert st == st2 == st3 == st4 == 0
    assert same_bits(a["G"], full["G"]) and same_bits(a["loss"], full["loss"]) and same_bits(b["G"], full["G"]) and same_bits(d["loss"], full["loss"])


@pytest.mark.parametrize("c", [5, 256])
@pytest.mark.parametrize("n", [9, 300])
def test_ce_workspace_at_any_alignment(env, n, c):
    """The header: "the workspace pointer may have any alignment".  The queried size exactly, at byte offsets 1, 4 and 255 of a buffer
    of NaN bytes: the bits of the aligned run, and (run_ce) no byte outside the queried size changes."""
    X, t = general(800 + c + n, n, c)
    rows = np.arange(0, n, 2)
    for call, kw in (("plain", dict(colsum=False)), ("colsum", {}), ("partial", dict(n_total=2 * n)), ("rows", dict(rows=rows, n_total=n))):
        st, base = run_ce(env, X, t, call, **kw)
        assert st == 0
        for off in (1, 4, 255):
            st, a = run_ce(env, X, t, call, ws_off=off, **kw)
            assert st == 0, (call, off)
            assert same_bits(a["G"], base["G"]) and same_bits(a["cs"], base["cs"]) and same_bits(a["loss"], base["loss"]), (call, off)


# ------------------------------------------------------------------ 7. non-finite logits stay inside their row
@pytest.mark.parametrize("c", [5, 256])
@pytest.mark.parametrize("poison", [np.inf, np.nan, 100.0])
def test_ce_non_finite_logit_stays_in_its_row(env, c, poison):
    """No max-subtraction by contract: x = 100 overflows expf.  The poisoned row's gradient and the loss are non-finite, every other
    gradient row has the bits of the clean run, no error status."""
    n, r = 9, 4
    X, t = general(850 + c, n, c)
    st, clean = run_ce(env, X, t, "colsum")
    assert st == 0 and np.isfinite(clean["G"]).all() and np.isfinite(clean["loss"]).all()
    for col in ((t[r] + 1) % c, t[r]):                       # off the target, on the target
        Xp = X.copy()
        Xp[r, col] = poison
        for call, rows in (("colsum", None), ("rows", np.arange(n))):
            st, a = run_ce(env, Xp, t, call, rows=rows)
            assert st == 0
            keep = np.arange(n) != r
            assert same_bits(a["G"][keep], clean["G"][keep]), (poison, col, call)
            assert not np.isfinite(a["G"][r]).all() and not np.isfinite(a["loss"][0]), (poison, col, call)
    # -inf off the target is an ordinary dead class: probability 0, everything finite and inside the bounds
    Xp = X.copy()
    Xp[r, (t[r] + 1) % c] = -np.inf
    st, a = run_ce(env, Xp, t, "colsum")
    assert st == 0 and np.isfinite(a["G"]).all() and np.isfinite(a["loss"][0]) and a["G"][r, (t[r] + 1) % c] == 0.0
    check_general(a, Xp, t, None, n, c == 256, f"-inf off the target C={c}")


# ------------------------------------------------------------------ 8. binary cross-entropy
def run_bce(env, x, y, n_total, loss=True, grad=True):
    torch, L, dv = env["torch"], env["L"], env["dev"]
    n = len(x)
    xd, yd = torch.from_numpy(np.ascontiguousarray(x)).to(dv), torch.from_numpy(np.ascontiguousarray(y)).to(dv)
    lbuf = torch.full((3,), float("nan"), dtype=torch.float32, device=dv)
    gbuf = torch.full((n + 2,), float("nan"), dtype=torch.float32, device=dv)
    need = C.c_size_t(0)
    assert L.gnnx_bce_logits_workspace(n, C.byref(need)) == 0
    ws = torch.full((need.value + 64,), 0xFF, dtype=torch.uint8, device=dv)
    st = L.gnnx_bce_logits_f32(xd.data_ptr(), yd.data_ptr(), n, n_total, (lbuf.data_ptr() + 4) if loss else None,
                               (gbuf.data_ptr() + 4) if grad else None, ws.data_ptr(), need.value, None)
    torch.cuda.synchronize()
    assert st == 0
    lh, gh = lbuf.cpu().numpy(), gbuf.cpu().numpy()
    assert np.all(ws.cpu().numpy()[need.value:] == 0xFF)
    assert bits(lh)[0] == NAN_BITS and bits(lh)[2] == NAN_BITS and bits(gh)[0] == NAN_BITS and bits(gh)[-1] == NAN_BITS
    assert loss or bits(lh)[1] == NAN_BITS
    assert grad or np.all(bits(gh) == NAN_BITS)
    return lh[1:2].copy(), gh[1:-1].copy()


def bce_general(n):
    x = synth.uniform_pm1(81, (n,), scale=6.0)
    y = (synth.uniform_pm1(82, (n,)) > 0).astype(np.float32)
    soft = np.arange(n) % 5 == 3
    y[soft] = (synth.uniform_pm1(83, (n,))[soft] + 1) / 2
    xs = np.array([30, -30, 88, 100, 0, 30, -30, 88, 100, 0, -88, -100, -88, -100], dtype=np.float32)
    ys = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0.25, 0.25], dtype=np.float32)     # (-88, -100 with y > 0: module docstring)
    m = min(n, len(xs))
    x[n - m:], y[n - m:] = xs[:m], ys[:m]
    return x, y.astype(np.float32)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65535, 65536, 65537, 131073])
def test_bce_logits(env, n):
    """bce_logits_kernel: 256 groups x 256 threads = 65536 elements a sweep."""
    n_total = 1 << 18
    x, y = lr.bce_dyadic(n, n)
    total, g = lr.bce_dyadic_int(x, y)
    loss, d = run_bce(env, x, y, n_total)
    assert np.array_equal(bits(loss), bits(np.array([total / n_total]))), f"dyadic loss n={n}: {loss[0]!r} vs {total / n_total!r}"
    assert np.array_equal(bits(d), bits(g / n_total)), f"dyadic gradient n={n}"
    l1, none = run_bce(env, x, y, n_total, grad=False)
    none2, d1 = run_bce(env, x, y, n_total, loss=False)
    assert same_bits(l1, loss) and same_bits(d1, d)
    xz, yz = lr.bce_dyadic(n + 1, n, with_zero=True)
    _, gz = lr.bce_dyadic_int(xz, yz)
    _, dz = run_bce(env, xz, yz, n_total, loss=False)
    assert np.array_equal(bits(dz), bits(gz / n_total)), f"dyadic gradient with x = 0, n={n}"
    x, y = bce_general(n)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for nt in (n, 2 * n + 1):
        loss_ref, g_ref = lr.bce_ref64(x, y, nt)
        loss, d = run_bce(env, x, y, nt)
        sig = 1.0 / (1.0 + np.exp(-x64))
        ratio = float((np.abs(d.astype(np.float64) - g_ref / nt) / (U * (sig + y64) / nt)).max())
        note("bce", "gradient", ratio, 6.0)
        assert ratio <= 6.0, f"n={n} n_total={nt}: gradient error / (2^-24 (sigmoid + y) / n_total) = {ratio:.3f} > 6"
        a = np.maximum(x64, 0) + np.abs(x64 * y64) + np.log1p(np.exp(-np.abs(x64)))
        depth = 9 + -(-n // 65536) + 8 + 256 + 2
        err = abs(float(loss[0]) - loss_ref)
        note("bce", "loss/sum", err / (U * a.sum() / nt), depth)
        print(f"n={n} n_total={nt}: bce loss {loss[0]:.9g} ref {loss_ref:.9g}, gradient ratio {ratio:.3f}, loss ratio {err / (U * a.sum() / nt):.3f}")
        assert err <= U * depth * a.sum() / nt
        l1, _ = run_bce(env, x, y, nt, grad=False)
        _, d1 = run_bce(env, x, y, nt, loss=False)
        assert same_bits(l1, loss) and same_bits(d1, d)
