"""GPU tests of the edge-score entry points (run with -m gpu on an MI355X): gnnx_sddmm_csr_f32 against the NumPy restatement of its
documented summation order (tests/sddmm_ref.py) BIT FOR BIT at every width of sddmm_ref.WIDTHS -- every lane group from 1 to 64,
idle lanes, a ragged last chunk, 2, 3 and 4 chunks per lane -- on patterns that put rows and runs of rows across any power-of-two
entries-per-wavefront boundary; its second use as the gradient of the aggregation's per-entry values; gnnx_csr_transpose_map;
gnnx_bce_logits_f32.

Bars (none is new): bit equality (torch.equal) for the scores and the index work; tests.helpers.assert_close against float64 --
1e-5 * max(1, |ref|[, absum]) with absum = sum_f |term_f| for a dot product (tests/test_sddmm_cpu.py says why the plain bar does not
fit one) -- for the gradient of the values and the loss."""
import functools
import importlib

import numpy as np
import pytest

from tests import sddmm_ref as sr
from tests.helpers import assert_close, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ patterns
def csr_from_lengths(lengths, n_cols, seed):
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.permutation(n_cols)[:k]) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rowptr, colidx


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(rowptr, colidx, n_rows, n_cols) as host arrays, ascending columns, no duplicates."""
    if name == "boundaries":
        # 0, 0, 1, then k - 1, k, k + 1 for every power of two k from 32 to 1024, empty rows between them and at both ends
        lengths = [0, 0, 1]
        for k in (32, 64, 128, 256, 512, 1024):
            lengths += [k - 1, 0, k, k + 1, 0, 0]
        rowptr, colidx = csr_from_lengths(lengths + [0], 1200, 41)
        return rowptr, colidx, len(lengths) + 1, 1200
    if name == "rmat":
        n = 1 << 12
        src, dst = synth.rmat_edges(43, n, 60_000, a=0.45, b=0.40, c=0.10)   # rows far more skewed than columns: long hub rows
        key = np.unique(src.astype(np.int64) * n + dst)
        rowptr = np.zeros(n + 1, dtype=np.int64)
        np.add.at(rowptr, key // n + 1, 1)
        rowptr = np.cumsum(rowptr).astype(np.int32)
        assert (np.diff(rowptr) > 1000).sum() >= 10 and np.diff(rowptr).max() > 3000   # hub rows of thousands of entries
        return rowptr, (key % n).astype(np.int32), n, n
    if name == "rect":
        rowptr, colidx = sr.random_csr(47, 150, 333, 3000)
        return rowptr, colidx, 150, 333
    if name == "one_row":
        rowptr, colidx = csr_from_lengths([77], 100, 53)
        return rowptr, colidx, 1, 100
    raise KeyError(name)


PATTERNS = ("boundaries", "rmat", "rect", "one_row")


@functools.lru_cache(maxsize=None)
def operands(name, F):
    _, _, n_rows, n_cols = pattern(name)
    L = synth.uniform_pm1(7000 + F, (n_rows, F))
    R = synth.uniform_pm1(9000 + F, (n_cols, F))
    rs = synth.uniform_pm1(11, (n_rows,)) + np.float32(1.5)
    cs = synth.uniform_pm1(13, (n_cols,)) - np.float32(1.5)
    return L, R, rs.astype(np.float32), cs.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, F):
    """The unscaled scores in the documented order: computed once per (pattern, width), shared, never written."""
    rowptr, colidx, _, _ = pattern(name)
    L, R, _, _ = operands(name, F)
    out = sr.sddmm_ref(rowptr, colidx, L, R)
    out.setflags(write=False)
    return out


def device_pattern(env, name):
    rowptr, colidx, _, _ = pattern(name)
    return dev(env, rowptr), dev(env, colidx)


# ------------------------------------------------------------------ 1. the scores, bit for bit
@pytest.mark.parametrize("F", sr.WIDTHS)
@pytest.mark.parametrize("name", PATTERNS)
def test_sddmm_bits_equal_the_documented_order(env, name, F):
    ops, torch = env["ops"], env["torch"]
    rp, ci = device_pattern(env, name)
    L, R, _, _ = operands(name, F)
    got = ops.sddmm(rp, ci, dev(env, L), dev(env, R))
    ref = torch.from_numpy(np.array(reference(name, F)))
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(got.cpu(), ref), f"{name} F={F}: {int((got.cpu() != ref).sum())} of {ref.numel()} entries differ"


SOME_WIDTHS = (3, 4, 33, 128, 256, 260, 516)   # scalar and vec4 rows, one and several chunks per lane


@pytest.mark.parametrize("F", SOME_WIDTHS)
@pytest.mark.parametrize("name", ("boundaries", "rmat"))
def test_sddmm_scales_pitch_and_unaligned_views(env, name, F):
    """rowscale, colscale, both (each a separately rounded multiply of the unscaled bits, row scale first); rows on a pitch ld > F;
    L or R as a view offset by one float (fails the 16-byte condition: scalar loads, same bits); two runs give equal bits."""
    ops, torch = env["ops"], env["torch"]
    rp, ci = device_pattern(env, name)
    rowptr, colidx, n_rows, n_cols = pattern(name)
    L, R, rs, cs = operands(name, F)
    rows, cols = sr.row_of_entries(rowptr), colidx.astype(np.int64)
    base = np.array(reference(name, F))
    dL, dR, drs, dcs = dev(env, L), dev(env, R), dev(env, rs), dev(env, cs)
    eq = lambda got, ref, what: torch.equal(got.cpu(), torch.from_numpy(ref)) or pytest.fail(f"{name} F={F}: {what} differs")  # noqa: E731
    eq(ops.sddmm(rp, ci, dL, dR, rowscale=drs), base * rs[rows], "rowscale")
    eq(ops.sddmm(rp, ci, dL, dR, colscale=dcs), base * cs[cols], "colscale")
    both = ops.sddmm(rp, ci, dL, dR, rowscale=drs, colscale=dcs)
    eq(both, (base * rs[rows]) * cs[cols], "both scales")
    assert torch.equal(both, ops.sddmm(rp, ci, dL, dR, rowscale=drs, colscale=dcs)), "two runs differ"
    # the gather pitch: rows on ld = F + 64 (16-byte aligned) and on ld = F + 3 (not)
    for pad in (64, 3):
        Lp = torch.full((n_rows, F + pad), float("nan"), device=env["dev"])
        Rp = torch.full((n_cols, F + pad), float("nan"), device=env["dev"])
        Lp[:, :F], Rp[:, :F] = dL, dR
        eq(ops.sddmm(rp, ci, Lp[:, :F], Rp[:, :F]), base, f"ld = F + {pad}")
    # views that start one float into a buffer
    for which in ("L", "R"):
        flat = torch.empty((n_rows if which == "L" else n_cols) * F + 1, device=env["dev"])
        view = flat[1:].view(-1, F)
        view.copy_(dL if which == "L" else dR)
        assert view.data_ptr() % 16 == 4
        eq(ops.sddmm(rp, ci, view if which == "L" else dL, view if which == "R" else dR), base, f"{which} offset by one float")
    out = torch.full((base.shape[0],), float("nan"), device=env["dev"])
    assert ops.sddmm(rp, ci, dL, dR, out=out) is out
    eq(out, base, "out=")


@pytest.mark.parametrize("F", (5, 16, 128, 256, 1024))
def test_sddmm_L_is_R(env, F):
    """Link scores <Z[i], Z[c]>: both operands the same tensor."""
    ops, torch = env["ops"], env["torch"]
    rp, ci = device_pattern(env, "rmat")
    rowptr, colidx, n, _ = pattern("rmat")
    Z = synth.uniform_pm1(300 + F, (n, F))
    dZ = dev(env, Z)
    assert torch.equal(ops.sddmm(rp, ci, dZ, dZ).cpu(), torch.from_numpy(sr.sddmm_ref(rowptr, colidx, Z, Z)))


def test_sddmm_empty_pattern_and_zero_width(env):
    ops, torch = env["ops"], env["torch"]
    rp0 = torch.zeros(6, dtype=torch.int32, device=env["dev"])
    ci0 = torch.empty(0, dtype=torch.int32, device=env["dev"])
    X = torch.ones((5, 8), device=env["dev"])
    assert ops.sddmm(rp0, ci0, X, X).numel() == 0                                     # nnz = 0: OK, nothing launched
    rp, ci = device_pattern(env, "rect")
    _, colidx, n_rows, n_cols = pattern("rect")
    out = torch.full((len(colidx),), float("nan"), device=env["dev"])
    rs = torch.full((n_rows,), -1.0, device=env["dev"])
    ops.sddmm(rp, ci, torch.empty((n_rows, 0), device=env["dev"]), torch.empty((n_cols, 0), device=env["dev"]), rowscale=rs, out=out)
    assert torch.equal(out.view(torch.int32), torch.zeros_like(out, dtype=torch.int32))   # n_feat = 0: +0 everywhere
    with pytest.raises(env["capi"].GnnxError):
        ops.sddmm(rp, ci, X, X)                                                           # L has the wrong number of rows


# ------------------------------------------------------------------ 2. the gradient of the aggregation's values
def test_spmm_vals_grad_vs_float64_autograd(env):
    """Y = rowscale (.) sum_p vals[p] colscale[c_p] X[c_p,:], loss = sum(G (.) Y): dloss/dvals from torch float64 autograd of the DENSE
    formulation on the CPU (the reference's G . X^T, operation.h:516-523, read at the stored entries)."""
    ops, torch = env["ops"], env["torch"]
    n, F = 200, 48
    rowptr, colidx = sr.random_csr(61, n, n, 3000)
    rows, cols = sr.row_of_entries(rowptr), colidx.astype(np.int64)
    vals = synth.uniform_pm1(62, (len(colidx),))
    X, G = synth.uniform_pm1(63, (n, F)), synth.uniform_pm1(64, (n, F))
    rs, cs = synth.uniform_pm1(65, (n,)) + np.float32(1.5), synth.uniform_pm1(66, (n,)) + np.float32(1.5)
    v = torch.from_numpy(vals).double().requires_grad_(True)
    A = torch.zeros((n, n), dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(cols)), v)
    t64 = lambda a: torch.from_numpy(a).double()  # noqa: E731
    Y = t64(rs)[:, None] * (A @ (t64(cs)[:, None] * t64(X)))
    (t64(G) * Y).sum().backward()
    terms = np.abs(G.astype(np.float64)[rows] * X.astype(np.float64)[cols]).sum(1) * np.abs(rs.astype(np.float64)[rows] * cs.astype(np.float64)[cols])
    got = ops.spmm_vals_grad(dev(env, rowptr), dev(env, colidx), dev(env, G), dev(env, X), rowscale=dev(env, rs), colscale=dev(env, cs))
    assert_close(host(got), v.grad.numpy(), "dL/dvals", absum=terms)
    # and it is the sddmm call under its second name: the documented bits
    assert np.array_equal(host(got), sr.sddmm_ref(rowptr, colidx, G, X, rowscale=rs, colscale=cs))
    # the forward it differentiates is the library's aggregation
    Yg = ops.spmm(dev(env, rowptr), dev(env, colidx), dev(env, X), vals=dev(env, vals), colscale=dev(env, cs), rowscale=dev(env, rs))
    assert_close(host(Yg), Y.detach().numpy(), "Y", absum=(np.abs(A.detach().numpy()) @ np.abs(cs[:, None] * X).astype(np.float64)) * np.abs(rs)[:, None])


# ------------------------------------------------------------------ 3. the position map
@pytest.mark.parametrize("name", PATTERNS)
def test_transpose_map_equals_reference(env, name):
    ops, torch = env["ops"], env["torch"]
    rowptr, colidx, n_rows, n_cols = pattern(name)
    rowptr_t, colidx_t = sr.transpose_csr(rowptr, colidx, n_cols)
    m = ops.csr_transpose_map(dev(env, rowptr), dev(env, colidx), dev(env, rowptr_t), dev(env, colidx_t))
    assert m.dtype == torch.int32
    ref = sr.transpose_map_ref(rowptr, colidx, rowptr_t, colidx_t)
    assert np.array_equal(host(m), ref)
    assert np.array_equal(np.sort(ref), np.arange(len(colidx)))                  # a permutation of the positions
    vals = synth.uniform_pm1(71, (len(colidx),))
    moved = ops.gather_rows(dev(env, vals).reshape(-1, 1), m).reshape(-1)        # the 1-column gather that carries values over
    assert np.array_equal(host(moved), vals[ref])


def test_transpose_map_refuses_what_is_not_a_sorted_transpose(env):
    ops, capi = env["ops"], env["capi"]
    rowptr, colidx, n_rows, n_cols = pattern("rect")
    rowptr_t, colidx_t = sr.transpose_csr(rowptr, colidx, n_cols)
    d = lambda a: dev(env, a)  # noqa: E731

    def status(*a):
        with pytest.raises(capi.GnnxError) as ei:
            ops.csr_transpose_map(*a)
        return ei.value.status

    # a row with descending columns (a relabelled graph stored in original-id order looks like this)
    r = int(np.argmax(np.diff(rowptr) >= 3))
    rev = colidx.copy()
    rev[rowptr[r]:rowptr[r + 1]] = rev[rowptr[r]:rowptr[r + 1]][::-1]
    assert status(d(rowptr), d(rev), d(rowptr_t), d(colidx_t)) == -3
    # a "transpose" with one entry moved to a row the pattern does not store
    c = int(np.argmax(np.diff(rowptr_t) >= 1))
    stored = set(colidx_t[rowptr_t[c]:rowptr_t[c + 1]].tolist())
    q = int(rowptr_t[c + 1]) - 1
    free = next(x for x in range(int(colidx_t[q]) + 1, n_rows + 1) if x not in stored)
    assert free < n_rows
    moved = colidx_t.copy()
    moved[q] = free                                                              # still ascending; (free, c) is not in the pattern
    assert (free, c) not in set(zip(sr.row_of_entries(rowptr).tolist(), colidx.tolist()))
    assert status(d(rowptr), d(colidx), d(rowptr_t), d(moved)) == -3
    # entry counts that disagree
    short = rowptr_t.copy()
    short[-1] -= 1
    assert status(d(rowptr), d(colidx), d(short), d(colidx_t)) == -3


# ------------------------------------------------------------------ 4. the loss over scored pairs
def bce_case(n):
    x = synth.uniform_pm1(81, (n,), scale=6.0)
    y = (synth.uniform_pm1(82, (n,)) > 0).astype(np.float32)
    special = np.array([30, -30, 88, -88, 100, -100, 0, 30, -30, 88, -88, 100, -100, 0], dtype=np.float32)[:n]
    x[:len(special)] = special
    y[:len(special)] = (np.arange(len(special)) >= 7).astype(np.float32)      # each special score with label 0 and label 1
    soft = np.arange(n) % 5 == 3
    y[soft] = (synth.uniform_pm1(83, (n,))[soft] + 1) / 2                        # soft targets in [0, 1]
    return x, y.astype(np.float32)


@pytest.mark.parametrize("n", [1, (1 << 20) + 3])
def test_bce_logits_vs_float64(env, n):
    ops, torch = env["ops"], env["torch"]
    x, y = bce_case(n)
    dx, dy = dev(env, x), dev(env, y)
    for n_total in (None, 2 * n + 1):
        loss_ref, g_ref = sr.bce_logits_ref64(x, y, n_total)
        loss, d = ops.bce_logits(dx, dy, n_total=n_total)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
        assert_close(host(loss).astype(np.float64), np.array([loss_ref]), f"loss n={n}")
        assert_close(host(d).astype(np.float64) * (n if n_total is None else n_total), g_ref, f"n_total * dscores n={n}")
        loss2, d2 = ops.bce_logits(dx, dy, n_total=n_total)
        assert torch.equal(loss, loss2) and torch.equal(d, d2), "two runs differ"
        loss3, none = ops.bce_logits(dx, dy, want_grad=False, n_total=n_total)
        assert none is None and torch.equal(loss3, loss)
    with pytest.raises(env["capi"].GnnxError) as ei:
        ops.bce_logits(dx[:0], dy[:0])
    assert ei.value.status == -1
