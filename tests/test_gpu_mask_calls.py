"""GPU tests of the label-mask calls of gnnx_masked.hip (run with -m gpu on an MI355X): gnnx_mask_to_rows, gnnx_csr_restrict,
gnnx_argmax_rows_f32 and gnnx_accuracy_rows_f32 through the C-ABI on sentinel-filled buffers, array-equal to the plain-loop
restatements of tests/loss_ref.py, at every chunk edge (64 mask bytes / 64 entries a wavefront, 4 rows a workgroup, 4096 workgroups a
sweep of the argmax) and on the tiny CSR patterns named for their edge.  tests/test_gpu_masked.py holds the workload shapes."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import loss_ref as lr
from tests.helpers import pkg  # noqa: F401  (registers the in-tree package under its importable alias)

pytestmark = pytest.mark.gpu

SENT = -77          # int32 sentinel of index outputs
FSENT = -77.5       # float sentinel of value outputs


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, capi=capi, L=capi.lib(), dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def workspace(env, query, *args):
    need = C.c_size_t(0)
    assert getattr(env["L"], query)(*args, C.byref(need)) == 0
    return env["torch"].full((need.value + 64,), 0xFF, dtype=env["torch"].uint8, device=env["dev"]), need.value


def masks(seed, n):
    """The mask kinds of the issue: all-drop, all-keep, first only, last only, alternating, seeded with set bytes from {1, 2, 0x80, 0xFF}."""
    rng = np.random.default_rng(seed)
    first, last, alt = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    if n:
        first[0], last[-1] = 1, 0xFF
    alt[::2] = 2
    out = {"zero": np.zeros(n, dtype=np.uint8), "one": np.ones(n, dtype=np.uint8), "first": first, "last": last, "alternating": alt}
    for j, density in enumerate((0.1, 0.5, 0.9)):
        set_bytes = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)[rng.integers(0, 4, n)]
        out[f"seeded{j}"] = np.where(rng.random(n) < density, set_bytes, 0).astype(np.uint8)
    return out


# ------------------------------------------------------------------ 1. mask -> rows
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_mask_to_rows(env, n):
    torch, L = env["torch"], env["L"]
    for name, m in masks(n, n).items():
        ref = lr.mask_rows_ref(m)
        rows = torch.full((n + 2,), SENT, dtype=torch.int32, device=env["dev"])
        ws, need = workspace(env, "gnnx_mask_to_rows_workspace", n)
        count = C.c_int32(-5)
        md = dev(env, m)
        st = L.gnnx_mask_to_rows(md.data_ptr(), n, rows.data_ptr() + 4, C.byref(count), ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        got = rows.cpu().numpy()
        assert st == 0 and count.value == len(ref), (n, name)
        assert np.array_equal(got[1:1 + len(ref)], ref), (n, name)
        assert np.all(got[1 + len(ref):] == SENT) and got[0] == SENT, f"n={n} {name}: a slot behind the count was written"
        assert np.all(ws.cpu().numpy()[need:] == 0xFF)
        assert np.array_equal(md.cpu().numpy(), m)


# ------------------------------------------------------------------ 2. CSR restriction
def run_restrict(env, n_rows, n_cols, rowptr, colidx, vals, row_keep, col_keep, nnz=None, in_place=False, vals_out=True):
    torch, L, dv = env["torch"], env["L"], env["dev"]
    nnz = len(colidx) if nnz is None else nnz
    cap = len(colidx)
    rp, ci = dev(env, rowptr), dev(env, colidx if cap else np.zeros(1, dtype=np.int32))
    rp_out = torch.full((n_rows + 3,), SENT, dtype=torch.int32, device=dv)
    ci_out = torch.full((cap + 2,), SENT, dtype=torch.int32, device=dv)
    v = None if vals is None else dev(env, vals if cap else np.zeros(1, dtype=np.float32))
    v_out = torch.full((cap + 2,), FSENT, dtype=torch.float32, device=dv)
    rk, ck = None if row_keep is None else dev(env, row_keep), None if col_keep is None else dev(env, col_keep)
    ws, need = workspace(env, "gnnx_csr_restrict_workspace", n_rows, max(nnz, 0))
    out_n = C.c_int64(-5)
    st = L.gnnx_csr_restrict(n_rows, n_cols, nnz, rp.data_ptr(), ci.data_ptr(), None if v is None else v.data_ptr(),
                             None if rk is None else rk.data_ptr(), None if ck is None else ck.data_ptr(),
                             rp.data_ptr() if in_place else rp_out.data_ptr() + 4, ci_out.data_ptr() + 4,
                             (v_out.data_ptr() + 4) if (vals is not None and vals_out) else None, C.byref(out_n), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert np.all(ws.cpu().numpy()[need:] == 0xFF)
    assert np.array_equal(rp.cpu().numpy(), rowptr) and (not cap or np.array_equal(ci.cpu().numpy(), colidx))
    return st, out_n.value, rp_out.cpu().numpy(), ci_out.cpu().numpy(), v_out.cpu().numpy()


def check_restrict(env, pat, row_keep, col_keep, with_vals, what):
    n_rows, n_cols, rowptr, colidx = pat
    vals = lr.tiny_vals(len(colidx)) if with_vals else None
    erp, eci, ev = lr.restrict_ref(rowptr, colidx, vals, row_keep, col_keep)
    st, k, rp, ci, v = run_restrict(env, n_rows, n_cols, rowptr, colidx, vals, row_keep, col_keep)
    assert st == 0 and k == len(eci), what
    assert np.array_equal(rp[1:n_rows + 2], erp) and rp[0] == SENT and rp[-1] == SENT, what
    assert np.array_equal(ci[1:1 + k], eci), what
    assert np.all(ci[1 + k:] == SENT) and ci[0] == SENT, f"{what}: a colidx slot behind nnz_out was written"
    if with_vals:
        assert np.array_equal(v[1:1 + k], ev), what
        assert np.all(v[1 + k:] == FSENT) and v[0] == FSENT, f"{what}: a vals slot behind nnz_out was written"
    else:
        assert np.all(v == FSENT), what


@pytest.mark.parametrize("name", sorted(lr.tiny_csr_patterns()))
def test_csr_restrict_tiny_patterns(env, name):
    pat = lr.tiny_csr_patterns()[name]
    n_rows, n_cols = pat[0], pat[1]
    kinds = ("one", "zero", "alternating", "seeded1")
    rms, cms = masks(31, n_rows), masks(32, n_cols)
    pairs = [(None, None)] + [(rms[a], None) for a in kinds] + [(None, cms[b]) for b in kinds] + [(rms[a], cms[b]) for a in kinds for b in kinds]
    for j, (rk, ck) in enumerate(pairs):
        for with_vals in (True, False):
            check_restrict(env, pat, rk, ck, with_vals, f"{name} mask pair {j} vals={with_vals}")


def test_csr_restrict_refusals(env):
    n_rows, n_cols, rowptr, colidx = lr.tiny_csr_patterns()["straddle"]
    vals = lr.tiny_vals(len(colidx))
    rk, ck = masks(33, n_rows)["alternating"], masks(34, n_cols)["seeded1"]
    for bad, where in ((n_cols, 0), (-1, 0), (n_cols, len(colidx) - 1), (-1, 130)):
        ci = colidx.copy()
        ci[where] = bad
        assert run_restrict(env, n_rows, n_cols, rowptr, ci, vals, None, ck)[0] == -3, (bad, where)
        assert run_restrict(env, n_rows, n_cols, rowptr, ci, vals, np.ones(n_rows, dtype=np.uint8), ck)[0] == -3, (bad, where)
        # "under a column mask": without one the ids are not looked at -- a plain copy, or the row mask's selection
        for row_keep in (None, rk):
            erp, eci, ev = lr.restrict_ref(rowptr, ci, vals, row_keep, None)
            st, k, rp, co, v = run_restrict(env, n_rows, n_cols, rowptr, ci, vals, row_keep, None)
            assert st == 0 and k == len(eci) and np.array_equal(rp[1:n_rows + 2], erp) and np.array_equal(co[1:1 + k], eci)
            assert np.array_equal(v[1:1 + k], ev)
    st, k, rp, co, v = run_restrict(env, n_rows, n_cols, rowptr, colidx, vals, rk, ck, nnz=len(colidx) - 1)
    assert st == -1 and k == 0 and np.all(rp == SENT) and np.all(co == SENT) and np.all(v == FSENT)
    st, k, rp, co, v = run_restrict(env, n_rows, n_cols, rowptr, colidx, vals, rk, ck, in_place=True)
    assert st == -1 and np.all(co == SENT) and np.all(v == FSENT)
    st, k, rp, co, v = run_restrict(env, n_rows, n_cols, rowptr, colidx, vals, rk, ck, vals_out=False)
    assert st == -1 and np.all(rp == SENT) and np.all(co == SENT)


# ------------------------------------------------------------------ 3. argmax / accuracy
ARGMAX_C = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
ARGMAX_CASES = [(n, c) for c in ARGMAX_C for n in (1, 4, 5)] + [(n, c) for c in (1, 65) for n in (16384, 16385, 32769)]


@pytest.mark.parametrize("n,c", ARGMAX_CASES)
def test_argmax_and_accuracy(env, n, c):
    torch, L, dv = env["torch"], env["L"], env["dev"]
    X = lr.argmax_case(c + n, n, c)
    ref = lr.argmax_first_ref(X)
    if c >= 63 and n >= 4:
        assert ((X == X.max(1, keepdims=True)).sum(1) > 1).any()               # ties are there
    ldx = c + 3
    Xd = torch.full((n, ldx), float("inf"), dtype=torch.float32, device=dv)    # a pad column that is read would win
    Xd[:, :c] = dev(env, X)
    ws, need = workspace(env, "gnnx_argmax_rows_workspace")
    pred = torch.full((n + 2,), SENT, dtype=torch.int32, device=dv)
    st = L.gnnx_argmax_rows_f32(Xd.data_ptr(), ldx, n, c, pred.data_ptr() + 4, ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    got = pred.cpu().numpy()
    assert st == 0 and np.array_equal(got[1:-1], ref) and got[0] == SENT and got[-1] == SENT
    # accuracy over every row: every third target wrong, targets of -1 and C never match
    t = ref.copy()
    t[np.arange(n) % 3 == 0] = (t[np.arange(n) % 3 == 0] + 1) % max(c, 2)
    t[np.arange(n) % 7 == 5] = -1
    t[np.arange(n) % 7 == 6] = c
    td = dev(env, t)
    correct = C.c_int64(-5)
    pred.fill_(SENT)
    st = L.gnnx_accuracy_rows_f32(Xd.data_ptr(), ldx, td.data_ptr(), None, n, n, c, pred.data_ptr() + 4, C.byref(correct), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert st == 0 and correct.value == int((t == ref).sum()) and np.array_equal(pred.cpu().numpy()[1:-1], ref)
    # the listed form: d_pred[k] is the class of the k-th listed row; slots behind n_listed stay
    rng = np.random.default_rng(n + c)
    for rows in (np.arange(0, n, 2), np.sort(rng.permutation(n)[:max(1, n // 3)]), np.array([n - 1])):
        rows = rows.astype(np.int32)
        nl = len(rows)
        rd = dev(env, rows)
        pred.fill_(SENT)
        correct = C.c_int64(-5)
        st = L.gnnx_accuracy_rows_f32(Xd.data_ptr(), ldx, td.data_ptr(), rd.data_ptr(), nl, n, c, pred.data_ptr() + 4, C.byref(correct),
                                      ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        got = pred.cpu().numpy()
        assert st == 0 and correct.value == int((t[rows] == ref[rows]).sum())
        assert np.array_equal(got[1:1 + nl], ref[rows]) and np.all(got[1 + nl:] == SENT) and got[0] == SENT
        correct = C.c_int64(-5)                                                # without d_pred: the count alone
        st = L.gnnx_accuracy_rows_f32(Xd.data_ptr(), ldx, td.data_ptr(), rd.data_ptr(), nl, n, c, None, C.byref(correct), ws.data_ptr(), need, None)
        assert st == 0 and correct.value == int((t[rows] == ref[rows]).sum())
    for bad in (-1, n):
        for where in (0, -1):
            rows = np.arange(0, n, 2).astype(np.int32)
            rows[where] = bad
            correct = C.c_int64(-5)
            st = L.gnnx_accuracy_rows_f32(Xd.data_ptr(), ldx, td.data_ptr(), dev(env, rows).data_ptr(), len(rows), n, c, None, C.byref(correct),
                                          ws.data_ptr(), need, None)
            assert st == -3, (bad, where)
    correct = C.c_int64(9)
    pred.fill_(SENT)
    st = L.gnnx_accuracy_rows_f32(Xd.data_ptr(), ldx, td.data_ptr(), td.data_ptr(), 0, n, c, pred.data_ptr() + 4, C.byref(correct), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert st == 0 and correct.value == 0 and np.all(pred.cpu().numpy() == SENT)
    assert np.all(ws.cpu().numpy()[need:] == 0xFF)
