"""GPU tests of the BatchNorm + ReLU kernels (gnn.cpp_amd/csrc/gnnx_norm.hip; run with -m gpu on an MI355X) against
tests/norm_ref.py: element arithmetic bit for bit, reductions by equality on data whose sums are exact in any order.

Which kernel and loop a shape reaches (F columns on a leading dimension ld, n rows):

  statistics (bn_stats, bn_partial) and the scalar backward sums: colreduce_stage1, fw = 1, 8, 64, 128, 256 columns per pass for
      F = 1, 7, 33, 100, >= 256; F = 300 takes two column passes, 1028 five.  ceil(n / 64) blocks up to 1024: n = 63, 64 -> one block,
      65 -> two; n = 65 537 -> 1024 blocks of 65 rows, of which the last 15 have no rows; n = 100 003 at F = 7 -> 98 rows per block,
      more than 3 * rpp = 96, so the four-rows-in-flight loop runs (everywhere else only its tail loop does).
  backward sums, 16-byte form (F % 4 == 0, F <= 1024, aligned): bn_bwd_vec_kernel<0>, q = F / 4 lanes per row, rpp = 256 / q rows per
      pass; 256 % q != 0 leaves dead lanes (F = 12: 1 lane, 100: 6, 300: 31, 1020: 1).  Same block counts as above.
  forward and backward apply, 16-byte form: bn_fwd_vec_kernel / bn_bwd_vec_kernel<1>, one block per 4 * rpp rows up to 8192 blocks:
      n = 4 rpp - 1, 4 rpp, 4 rpp + 1 -> a partial pass, a full pass, a second block; n = 32 771 at F = 1024 -> 8192 blocks of 5 rows,
      each loops twice.
  forward and backward apply, scalar form (odd ld, misaligned base, F % 4 != 0 or F > 1024): bn_fwd_kernel / bn_bwd_kernel, one
      thread per element up to 4096 blocks: n = 4 099 at F = 257 -> 4115 blocks' worth of elements, the grid wraps.

Every matrix sits in a buffer filled with a sentinel (pad columns, two rows behind the last one, the elements before a shifted
base); an output's sentinels must survive the call."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import norm_ref as R
from tests.helpers import Pitched          # (tests.helpers also registers the in-tree package)

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARG, WORKSPACE = -1, -4
LAYOUTS = ("x_off", "odd_ldx", "odd_ldy", "odd_ldd", "odd_ldo", "pitch4")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def host(t):
    return t.detach().cpu().numpy()


def vec(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(env["dev"])


def upload(env, c, n, F, pad=0, pads=None, offs=None):
    """The case's matrices as Pitched views (pads / offs per operand: x, y, d, o) and its column vectors on the device."""
    pads, offs = pads or {}, offs or {}
    p = lambda k: pads.get(k, pad)  # noqa: E731
    o = lambda k: offs.get(k, 0)  # noqa: E731
    return dict(X=Pitched(env["dev"], n, F, p("x"), o("x"), c["x"]), dY=Pitched(env["dev"], n, F, p("d"), o("d"), c["dy"]),
                mean=vec(env, c["mean"]), var=vec(env, c["var"]), gamma=vec(env, c["gamma"]), beta=vec(env, c["beta"]),
                new_y=lambda: Pitched(env["dev"], n, F, p("y"), o("y")), new_o=lambda: Pitched(env["dev"], n, F, p("o"), o("o")))


def forward(env, d, c, relu, gamma=True, beta=True, stats=True, what=""):
    """ops.bn_relu_fwd into a sentinel-filled output, held to the restatement; returns the output (Pitched)."""
    Y = d["new_y"]()
    env["ops"].bn_relu_fwd(d["X"].view, d["mean"] if stats else None, d["var"] if stats else None, d["gamma"] if gamma else None,
                           d["beta"] if beta else None, eps=c["eps"], relu=bool(relu), out=Y.view)
    ref = R.bn_fwd_ref(c["x"], c["mean"] if stats else None, c["var"] if stats else None, c["gamma"] if gamma else None,
                       c["beta"] if beta else None, c["eps"], relu)
    R.assert_bits(Y.get(), ref, f"{what} forward relu={relu} gamma={gamma} beta={beta} stats={stats}")
    Y.assert_untouched_outside(f"{what} forward")
    return Y


def backward(env, d, c, Y, relu=True, gamma=True, beta=True, quirk=False):
    """ops.bn_relu_bwd into a sentinel-filled dX; returns (dX host, dgamma host, dbeta host)."""
    out = d["new_o"]()
    _, dgamma, dbeta = env["ops"].bn_relu_bwd(d["X"].view, None if Y is None else Y.view, d["dY"].view, d["mean"], d["var"],
                                              d["gamma"] if gamma else None, eps=c["eps"], relu=bool(relu), beta=d["beta"] if beta else None,
                                              reference_quirk=quirk, out=out.view)
    out.assert_untouched_outside("backward dX")
    return out.get(), host(dgamma), host(dbeta)


def expected_backward(c, n_total, relu=True, gamma=True, beta=True, quirk=False, sums=None):
    """The restated backward.  sums None: the exact data's sums (asserted exact); else the (dgamma, dbeta) to apply with."""
    x, dy, mean, var, eps = c["x"], c["dy"], c["mean"], c["var"], c["eps"]
    gm, bt = c["gamma"] if gamma else None, c["beta"] if beta else None
    g = R.masked(dy, R.relu_mask_ref(x, None, mean, var, gm, bt, eps) if relu else None)
    if sums is None:
        t0, t1 = R.bn_bwd_terms(x, g, mean, var, eps)
        sums = (R.exact_colsum(t1), R.exact_colsum(t0))
    dgamma, dbeta = sums
    dx = R.bn_bwd_quirk_ref(g, var, gm, eps) if quirk else R.bn_bwd_apply_ref(x, g, mean, var, gm, dgamma, dbeta, n_total, eps)
    return dx, dgamma, dbeta


def check_backward(got, ref, what):
    R.assert_bits(got[0], ref[0], what + " dX")
    assert np.array_equal(got[1], ref[1]), f"{what} dgamma: {R.describe_mismatch(got[1], ref[1])}"
    assert np.array_equal(got[2], ref[2]), f"{what} dbeta: {R.describe_mismatch(got[2], ref[2])}"


def check_statistics(env, d, c, n):
    """bn_partial with scale 1 and 0.25 on both reductions, exact; bn_stats: the mean is float32(sum) * (1 / n), and (mean, var)
    are bit for bit the two bn_partial calls with scale = 1 / n and that mean."""
    ops, X = env["ops"], d["X"].view
    for scale in (1.0, 0.25):
        got = host(ops.bn_partial(X, None, scale))
        assert np.array_equal(got, R.exact_colsum(c["x"], scale=scale)), f"bn_partial sum, scale {scale}: {R.describe_mismatch(got, R.exact_colsum(c['x'], scale=scale))}"
        ref = R.exact_colsum(R.sqdev_terms(c["x"], c["mean"]), scale=scale)
        got = host(ops.bn_partial(X, d["mean"], scale))
        assert np.array_equal(got, ref), f"bn_partial centred squares, scale {scale}: {R.describe_mismatch(got, ref)}"
    mean, var = ops.bn_stats(X)
    inv_n = float(F32(1) / F32(n))
    assert np.array_equal(host(mean), R.bn_stats_mean_ref(c["x"])), "bn_stats mean"
    R.assert_bits(host(mean), host(ops.bn_partial(X, None, inv_n)), "bn_stats mean vs bn_partial")
    R.assert_bits(host(var), host(ops.bn_partial(X, mean, inv_n)), "bn_stats var vs bn_partial on its mean")
    return host(mean), host(var)


@pytest.mark.parametrize("cell", R.cells(), ids=R.cell_id)
def test_every_cell_on_exact_data(env, cell):
    """Statistics, forward, textbook and quirk backward with the stored forward output and without it, and the mask-only form, on the
    exact data: sums by equality with the float64 sums, elements bit for bit."""
    F, pad, n, _ = cell
    c = R.exact_case(n, F)
    d = upload(env, c, n, F, pad)
    check_statistics(env, d, c, n)
    forward(env, d, c, relu=0)
    Y = forward(env, d, c, relu=1)
    for quirk in (False, True):
        ref = expected_backward(c, n, quirk=quirk)
        stored, recomputed = backward(env, d, c, Y, quirk=quirk), backward(env, d, c, None, quirk=quirk)
        check_backward(stored, ref, f"quirk={quirk} stored Y")
        check_backward(recomputed, ref, f"quirk={quirk} Y=NULL")
    # mask only: no statistics, the sign of the stored output or of x itself
    out = d["new_o"]()
    env["ops"].bn_relu_bwd(d["X"].view, Y.view, d["dY"].view, relu=True, out=out.view)
    R.assert_bits(out.get(), R.masked(c["dy"], Y.get() > 0), "mask only, stored Y")
    out.assert_untouched_outside("mask only")
    out = d["new_o"]()
    env["ops"].bn_relu_bwd(d["X"].view, None, d["dY"].view, relu=True, out=out.view)
    R.assert_bits(out.get(), R.masked(c["dy"], c["x"] > 0), "mask only, Y=NULL")


@pytest.mark.parametrize("cell", R.APPLY_CELLS, ids=R.cell_id)
def test_grid_cap_cells_of_forward_and_apply(env, cell):
    """The shapes at which the forward and the apply kernels run out of blocks: sums are handed in (dyadic vectors), so only the two
    streaming kernels run."""
    F, pad, n, _ = cell
    c = R.exact_case(n, F)
    d = upload(env, c, n, F, pad)
    Y = forward(env, d, c, relu=1)
    dgamma, dbeta = R.GAMMA_VALUES[np.arange(F) % 5] * F32(64), R.X_VALUES[np.arange(F) % 4] * F32(32)
    n_total = 65_536
    ref = expected_backward(c, n_total, sums=(dgamma, dbeta))[0]
    for Yv in (Y, None):
        out = d["new_o"]()
        env["ops"].bn_relu_bwd_apply(d["X"].view, None if Yv is None else Yv.view, d["dY"].view, d["mean"], d["var"], d["gamma"], vec(env, dgamma),
                                     vec(env, dbeta), n_total, eps=c["eps"], relu=True, beta=d["beta"], out=out.view)
        R.assert_bits(out.get(), ref, "apply")
        out.assert_untouched_outside("apply")


@pytest.mark.parametrize("n", [1, 2, 64])
@pytest.mark.parametrize("F", [7, 33, 300])
def test_variance_is_exact_at_power_of_two_counts(env, n, F):
    x = R.exact_case(n, F)["x"]
    mean, var = env["ops"].bn_stats(vec(env, x))
    ref_mean = R.bn_stats_mean_ref(x)
    assert np.array_equal(host(mean), ref_mean)
    assert np.array_equal(host(var), R.exact_colsum(R.sqdev_terms(x, ref_mean), 2.0 ** -12, scale=1.0 / n))


RANDOM_CELLS = [(F, pad, n) for F, pad in R.SCALAR_WIDTHS + R.VECTOR_WIDTHS for n in sorted({65, min(R.row_counts(F, pad)[-1], 300), 300})]


@pytest.mark.parametrize("F,pad,n", RANDOM_CELLS, ids=lambda v: str(v))
def test_element_arithmetic_and_rounding_on_random_data(env, F, pad, n):
    """Real-valued data with made-up column statistics: forward and dX bit for bit against the restatement (dX given the kernel's
    own sums), Y = NULL equal to the stored Y, and the sums inside the any-order bound gamma_k * sum|term| against float64 on the same
    float32 inputs -- k = n for dbeta (n - 1 additions), n + 5 for dgamma (var + eps, sqrt, 1 / sigma, x - mean, * rstd, g * xhat, then
    n - 1 additions).  The statistics are held to k = n + 3 (x - mean, the square, n - 1 additions, 1 / n, the scaling): the figure
    the bound was set with.  A rigorous count for the variance is n + 4, because the subtraction's error enters the square twice; the
    test asserts the tighter n + 3.  n <= 300 throughout."""
    ops = env["ops"]
    c = R.random_case(n, F)
    d = upload(env, c, n, F, pad)
    # statistics: the kernel's own mean is the float32 mean the variance reference is evaluated on
    mean, var = (host(t) for t in ops.bn_stats(d["X"].view))
    x64 = c["x"].astype(np.float64)
    assert (np.abs(mean - x64.sum(0) / n) <= R.gamma_k(n + 3) * np.abs(x64).sum(0) / n).all(), "bn_stats mean"
    terms = (x64 - mean.astype(np.float64)) ** 2
    err, bound = np.abs(var - terms.sum(0) / n), R.gamma_k(n + 3) * terms.sum(0) / n
    assert (err <= bound).all(), f"bn_stats var: err / bound = {(err / bound).max():.3f}"
    for gamma, beta in ((True, True), (False, True), (True, False)):
        forward(env, d, c, relu=0, gamma=gamma, beta=beta)
        Y = forward(env, d, c, relu=1, gamma=gamma, beta=beta)
        for quirk in (False, True):
            stored = backward(env, d, c, Y, gamma=gamma, beta=beta, quirk=quirk)
            recomputed = backward(env, d, c, None, gamma=gamma, beta=beta, quirk=quirk)
            for a, b, what in zip(stored, recomputed, ("dX", "dgamma", "dbeta")):
                R.assert_bits(b, a, f"Y=NULL vs stored Y, quirk={quirk} gamma={gamma} beta={beta}: {what}")
            ref = expected_backward(c, n, gamma=gamma, beta=beta, quirk=quirk, sums=(stored[1], stored[2]))
            R.assert_bits(stored[0], ref[0], f"dX quirk={quirk} gamma={gamma} beta={beta}")
            g = R.masked(c["dy"], Y.get() > 0).astype(np.float64)
            xhat = (x64 - c["mean"].astype(np.float64)) / np.sqrt(c["var"].astype(np.float64) + np.float64(F32(c["eps"])))
            assert (np.abs(stored[2] - g.sum(0)) <= R.gamma_k(n) * np.abs(g).sum(0)).all(), "dbeta"
            t = g * xhat
            err, bound = np.abs(stored[1] - t.sum(0)), R.gamma_k(n + 5) * np.abs(t).sum(0)
            assert (err <= bound).all(), f"dgamma: err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}"


@pytest.mark.parametrize("F,pad,n", [(12, 0, 341), (256, 0, 65), (7, 0, 65), (256, 1, 65)], ids=lambda v: str(v))
@pytest.mark.parametrize("gamma,beta,relu", [(g, b, r) for g in (True, False) for b in (True, False) for r in (1, 0)])
def test_pointer_modes_on_exact_data(env, F, pad, n, gamma, beta, relu):
    """gamma / beta present or NULL, relu on or off, Y stored or NULL, on both paths: the exact data's +-0 columns are where a
    recomputed sign can go wrong."""
    c = R.exact_case(n, F, seed=3)
    d = upload(env, c, n, F, pad)
    Y = forward(env, d, c, relu=relu, gamma=gamma, beta=beta)
    for quirk in (False, True):
        ref = expected_backward(c, n, relu=relu, gamma=gamma, beta=beta, quirk=quirk)
        check_backward(backward(env, d, c, Y, relu=relu, gamma=gamma, beta=beta, quirk=quirk), ref, f"quirk={quirk} stored Y")
        check_backward(backward(env, d, c, None, relu=relu, gamma=gamma, beta=beta, quirk=quirk), ref, f"quirk={quirk} Y=NULL")
    forward(env, d, c, relu=relu, stats=False)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F", [64, 256])
def test_layout_cells(env, F, layout):
    """One failed 16-byte condition at a time (the scalar kernels), and an aligned pitch of F + 4 (still the 16-byte kernels)."""
    n = 67
    pads, offs = {}, {}
    if layout == "x_off":
        offs["x"] = 1
    elif layout == "pitch4":
        pads = dict(x=4, y=4, d=4, o=4)
    else:
        pads[layout[-1]] = 1
    c = R.exact_case(n, F, seed=5)
    d = upload(env, c, n, F, 0, pads, offs)
    forward(env, d, c, relu=0, what=layout)
    Y = forward(env, d, c, relu=1, what=layout)
    for quirk in (False, True):
        ref = expected_backward(c, n, quirk=quirk)
        check_backward(backward(env, d, c, Y, quirk=quirk), ref, f"{layout} quirk={quirk} stored Y")
        check_backward(backward(env, d, c, None, quirk=quirk), ref, f"{layout} quirk={quirk} Y=NULL")
    cr = R.random_case(n, F, seed=5)
    dr = upload(env, cr, n, F, 0, pads, offs)
    Yr = forward(env, dr, cr, relu=1, what=layout + " random")
    a, b = backward(env, dr, cr, Yr), backward(env, dr, cr, None)
    if layout != "odd_ldy":     # (there Y = NULL lifts the one failed condition: the two calls run different kernels, whose sums of
        for u, v in zip(a, b):  # real-valued data differ by rounding; each is held to the restatement on its own sums below)
            R.assert_bits(v, u, layout + " random: Y=NULL vs stored Y")
    for got in (a, b):
        R.assert_bits(got[0], expected_backward(cr, n, sums=(got[1], got[2]))[0], layout + " random dX")


@pytest.mark.parametrize("F,pad", [(12, 0), (256, 0), (7, 0), (100, 1)], ids=lambda v: str(v))
def test_sharded_halves(env, F, pad):
    """Rows split 100 / 241: the per-part sums add up (exactly, on the exact data) to the whole matrix's, the per-part apply with
    n_total = n gives the one-call dX rows, and n_total above n_rows (a power of two) gives the restated arithmetic."""
    ops, n, cut = env["ops"], 341, 100
    c = R.exact_case(n, F, seed=7)
    d = upload(env, c, n, F, pad)
    whole = backward(env, d, c, None)
    parts = []
    for r0, r1 in ((0, cut), (cut, n)):
        cp = dict(c, x=c["x"][r0:r1], dy=c["dy"][r0:r1])
        dp = upload(env, cp, r1 - r0, F, pad)
        Yp = forward(env, dp, cp, relu=1)
        for Yv in (Yp.view, None):
            dgamma, dbeta = ops.bn_relu_bwd_sums(dp["X"].view, Yv, dp["dY"].view, dp["mean"], dp["var"], dp["gamma"], eps=c["eps"], relu=True, beta=dp["beta"])
            ref = expected_backward(cp, n)
            assert np.array_equal(host(dgamma), ref[1]) and np.array_equal(host(dbeta), ref[2]), "sums of a part"
        parts.append((cp, dp, Yp, host(dgamma), host(dbeta)))
    dgamma, dbeta = parts[0][3] + parts[1][3], parts[0][4] + parts[1][4]
    assert np.array_equal(dgamma, whole[1]) and np.array_equal(dbeta, whole[2])
    for (cp, dp, Yp, _, _), (r0, r1) in zip(parts, ((0, cut), (cut, n))):
        for n_total in (n, 512):
            for Yv in (Yp.view, None):
                out = dp["new_o"]()
                ops.bn_relu_bwd_apply(dp["X"].view, Yv, dp["dY"].view, dp["mean"], dp["var"], dp["gamma"], vec(env, dgamma), vec(env, dbeta), n_total,
                                      eps=c["eps"], relu=True, beta=dp["beta"], out=out.view)
                out.assert_untouched_outside("apply of a part")
                R.assert_bits(out.get(), expected_backward(cp, n_total, sums=(dgamma, dbeta))[0], f"apply n_total={n_total}")
                if n_total == n:
                    R.assert_bits(out.get(), whole[0][r0:r1], "apply of a part vs the one-call dX")


def test_argument_errors_leave_the_outputs_alone(env):
    """Each documented refusal returns its status and writes nothing."""
    torch, L = env["torch"], env["capi"].lib()
    n, F = 10, 8
    c = R.exact_case(n, F)
    d = upload(env, c, n, F)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    X, dY, mean, var, gamma, beta = (ptr(t) for t in (d["X"].view, d["dY"].view, d["mean"], d["var"], d["gamma"], d["beta"]))
    wsb = C.c_size_t(0)
    assert L.gnnx_bn_workspace(n, F, C.byref(wsb)) == 0
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=env["dev"])
    outs = [Pitched(env["dev"], n, F) for _ in range(2)] + [Pitched(env["dev"], 1, F) for _ in range(2)]
    O, Y, v0, v1 = (ptr(o.view) for o in outs)

    def refused(status, expected, what):
        assert status == expected, f"{what}: status {status}, expected {expected}"
        torch.cuda.synchronize()
        for o in outs:
            o.assert_untouched(what)

    stats = lambda rows, ld, w, nbytes: L.gnnx_bn_stats_f32(X, ld, rows, F, v0, v1, w, nbytes, None)  # noqa: E731
    refused(stats(0, F, ptr(ws), wsb.value), INVALID_ARG, "bn_stats: empty batch")
    refused(stats(n, F - 1, ptr(ws), wsb.value), INVALID_ARG, "bn_stats: ld < F")
    refused(stats(n, F, ptr(ws), wsb.value - 1), WORKSPACE, "bn_stats: workspace one byte short")
    refused(L.gnnx_bn_partial_f32(X, F, n, F, None, 1.0, v0, ptr(ws), wsb.value - 1, None), WORKSPACE, "bn_partial: workspace one byte short")
    refused(L.gnnx_bn_partial_f32(X, F - 1, n, F, None, 1.0, v0, ptr(ws), wsb.value, None), INVALID_ARG, "bn_partial: ld < F")
    fwd = lambda ldx, ldy, m, v: L.gnnx_bn_relu_fwd_f32(X, ldx, n, F, m, v, 0.0, gamma, beta, 1, Y, ldy, None)  # noqa: E731
    refused(fwd(F - 1, F, mean, var), INVALID_ARG, "forward: ldx < F")
    refused(fwd(F, F - 1, mean, var), INVALID_ARG, "forward: ldy < F")
    refused(fwd(F, F, mean, None), INVALID_ARG, "forward: mean without var")
    refused(fwd(F, F, None, var), INVALID_ARG, "forward: var without mean")

    def bwd(name="gnnx_bn_relu_bwd_f32", rows=n, ldx=F, ldd=F, ldo=F, m=mean, v=var, nbytes=wsb.value, y=None, ldy=0, out=O):
        return getattr(L, name)(X, ldx, y, ldy, dY, ldd, rows, F, m, v, 0.0, gamma, beta, 1, out, ldo, v0, v1, ptr(ws), nbytes, None)

    stored = X      # any [n, F] matrix serves as the stored forward output of a call that must refuse
    for name in ("gnnx_bn_relu_bwd_f32", "gnnx_bn_relu_bwd_quirk_f32"):     # the refusals of the apply half come before the sums are written
        refused(bwd(name, ldo=F - 1), INVALID_ARG, f"{name}: ldo < F")
        refused(bwd(name, out=None), INVALID_ARG, f"{name}: dX is null")
        refused(bwd(name, y=stored, ldy=F - 1), INVALID_ARG, f"{name}: ldy < F with a stored Y")
        refused(bwd(name, ldx=F - 1), INVALID_ARG, f"{name}: ldx < F")
        refused(bwd(name, ldd=F - 1), INVALID_ARG, f"{name}: ldd < F")
        refused(bwd(name, rows=0), INVALID_ARG, f"{name}: empty batch")
    refused(bwd(m=None), INVALID_ARG, "backward: var without mean")
    refused(bwd(v=None), INVALID_ARG, "backward: mean without var")
    refused(bwd(nbytes=wsb.value - 1), WORKSPACE, "backward: workspace one byte short")
    refused(bwd("gnnx_bn_relu_bwd_quirk_f32", m=None, v=None), INVALID_ARG, "quirk without statistics")
    refused(bwd("gnnx_bn_relu_bwd_quirk_f32", nbytes=wsb.value - 1), WORKSPACE, "quirk: workspace one byte short")

    def apply(dg=v0, db=v1, n_total=n, ldo=F, nbytes=wsb.value, y=None, ldy=0):
        return L.gnnx_bn_relu_bwd_apply_f32(X, F, y, ldy, dY, F, n, F, mean, var, 0.0, gamma, beta, 1, dg, db, n_total, O, ldo, ptr(ws), nbytes, None)

    refused(apply(dg=None), INVALID_ARG, "apply: statistics without dgamma")
    refused(apply(db=None), INVALID_ARG, "apply: statistics without dbeta")
    refused(apply(n_total=n - 1), INVALID_ARG, "apply: n_total < n_rows")
    refused(apply(ldo=F - 1), INVALID_ARG, "apply: ldo < F")
    refused(apply(y=stored, ldy=F - 1), INVALID_ARG, "apply: ldy < F with a stored Y")
    refused(apply(nbytes=wsb.value - 1), WORKSPACE, "apply: workspace one byte short")
    refused(L.gnnx_bn_relu_bwd_sums_f32(X, F, None, 0, dY, F, n, F, None, None, 0.0, gamma, beta, 1, v0, v1, ptr(ws), wsb.value, None), INVALID_ARG,
            "sums without statistics")
    refused(L.gnnx_bn_relu_bwd_sums_f32(X, F, None, 0, dY, F, n, F, mean, var, 0.0, gamma, beta, 1, v0, v1, ptr(ws), wsb.value - 1, None), WORKSPACE,
            "sums: workspace one byte short")
    refused(L.gnnx_bn_relu_bwd_sums_f32(X, F, stored, F - 1, dY, F, n, F, mean, var, 0.0, gamma, beta, 1, v0, v1, ptr(ws), wsb.value, None), INVALID_ARG,
            "sums: ldy < F with a stored Y")
