"""GPU tests of the streaming kernels of gnn.cpp_amd/csrc/gnnx_elementwise.hip and of gnnx_sgd_step_f32 (run with -m gpu on an
MI355X) against tests/elementwise_ref.py: reductions by equality on data whose sums are exact in any order, element arithmetic and
data movement bit for bit, sentinels around every output.

Which kernel and loop a shape reaches:

  colsum / colsum_copy / rows_to_slots with sums: ceil(n / 64) row ranges up to 512 (two per CU).  colsum_stage1_vec for F % 4 == 0 with
      F / 4 a divisor of 256 on aligned rows (F = 4, 8, 64, 256, 1024); its unrolled loop needs more than 3 * 256 / (F / 4) rows in a
      range: at F = 4 that is 768, reached by n = 400 003 (782 rows per range).  colsum_stage1 for the other widths >= 128 (132, 300,
      1028; 256 on an odd ld), colsum_stage1_narrow below 128 (1, 7, 33, 100).  n = 63 -> 1 range, 65 and 127 -> 2, 129 -> 3, 70 001 ->
      the 512 cap.  The copy rides in the 16-byte kernel, two ranges per workgroup when the range count is even, one when it is odd;
      other widths copy with a strided memcpy behind the sums.
  rows_to_slots without sums: blocks of 256 rows.
  rowsum: one wavefront per row, lane l sums columns [l w, (l + 1) w), w = ceil(C / 64); 16 bytes at a time when w % 4 == 0 and the
      rows are aligned (C = 200, 252, 256, 1024; lanes past C / w have an empty slice at 200 and 252), else scalar (1, 63, 64, 65, 260,
      any odd ld).
  gather_rows / scatter_add_rows: 16-byte lanes for F % 4 == 0 on aligned pitches, else scalar; 4 .. 64 lanes per row, a row wider
      than its lanes loops (F = 1024, 100, 300).
  transpose: 32 x 32 tiles, all on grid.x: (2 097 185, 3) and (3, 2 097 185) have 65 537 of them along one side.
  axpy / fill / sgd_step: 2048 blocks of 256 threads sweep; n = 600 001 needs a second sweep."""
import functools
import importlib

import numpy as np
import pytest

from tests import elementwise_ref as E
from tests import norm_ref as R
from tests.helpers import SENTINEL, Pitched          # (tests.helpers also registers the in-tree package)

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


def host(t):
    return t.detach().cpu().numpy()


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def assert_equal(got, ref, what):
    assert np.array_equal(got, ref), f"{what}: {R.describe_mismatch(got, ref)}"


# ------------------------------------------------------------------------------------------------ column sums
@functools.lru_cache(maxsize=2)
def colsum_input(n, F):
    """The exact matrix of a shape, drawn once for the four betas that follow each other."""
    return E.exact_matrix(n, F)


def start_of(beta, F):
    """(the accumulator before the call, what the reference reads): beta == 0 must not read it, so it holds NaN."""
    out0 = E.exact_out(F)
    return (np.full(F, np.nan, dtype=np.float32), None) if beta == 0 else (out0, out0)


@pytest.mark.parametrize("beta", E.BETAS, ids=lambda b: f"beta{b}")
@pytest.mark.parametrize("F,pad,n,kernel", E.COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_and_colsum_copy(env, F, pad, n, kernel, beta):
    """out = beta * out + sum for beta in {0 (out full of NaN), 1, 0.5, -2}, by equality; colsum_copy: the same sums, the copy equal
    to the source on its own pitch, nothing written around it."""
    ops, torch = env["ops"], env["torch"]
    G = colsum_input(n, F)
    Gd = Pitched(env["dev"], n, F, pad, 0, G)
    start, out0 = start_of(beta, F)
    ref = E.colsum_ref(G, beta, out0)
    out = dev(env, start)
    ops.colsum(Gd.view, out=out, beta=beta)
    assert_equal(host(out), ref, f"colsum beta={beta}")
    for cpad in (4, 1):     # an aligned pitch (the copy rides in the 16-byte kernel when the sums do) and an odd one (the fallback)
        out, copy = dev(env, start), Pitched(env["dev"], max(n, 1), F, cpad)      # (no rows: a one-row buffer that must stay as it is)
        ops.colsum_copy(Gd.view, copy.view, out=out, beta=beta)
        assert_equal(host(out), ref, f"colsum_copy beta={beta} copy pitch F+{cpad}")
        assert torch.equal(copy.view[:n], Gd.view), f"colsum_copy: the copy differs from the source, pitch F+{cpad}"
        copy.assert_untouched_outside("colsum_copy")
        assert n or bool((copy.buf == SENTINEL).all()), "colsum_copy of no rows wrote to the copy"
    assert torch.equal(Gd.view, dev(env, G)), "the source changed"


@pytest.mark.parametrize("beta", (None,) + E.BETAS, ids=lambda b: "nosums" if b is None else f"beta{b}")
@pytest.mark.parametrize("per_row", [(0,), (1,), (7,), (0, 1, 7, 0, 2)], ids=lambda v: "slots" + "".join(map(str, v)))
@pytest.mark.parametrize("F", E.SLOT_WIDTHS)
def test_rows_to_slots(env, F, per_row, beta):
    """The producer-side pack: the send buffer equals the gather pack (and the loop restatement), rows nobody wants go nowhere,
    and the sums from the same pass (beta not None) are colsum's bits and the exact sums."""
    ops, torch = env["ops"], env["torch"]
    for n in E.SLOT_ROWS:
        X = E.exact_matrix(n, F, seed=1)
        send_idx = E.send_list(n, per_row, seed=F)
        table = E.slot_table_ref(send_idx, n)
        assert np.array_equal(host(ops.slot_table(dev(env, send_idx), n)), table)
        Xd, td, n_slots = Pitched(env["dev"], n, F, 4, 0, X), dev(env, table), len(send_idx)
        n_send = max(n_slots, 1)                    # (no slots at all: a one-row send buffer that must stay as it is)
        ref = E.rows_to_slots_ref(X, table, n_send, SENTINEL)
        if n_slots:
            assert np.array_equal(ref, E.gather_ref(X, send_idx))
        send = Pitched(env["dev"], n_send, F, 4)
        if beta is None:
            ops.rows_to_slots(Xd.view, td, send.view)
        else:
            start, out0 = start_of(beta, F)
            out, plain = dev(env, start), dev(env, start)
            ops.rows_to_slots(Xd.view, td, send.view, colsum_out=out, beta=beta)
            ops.colsum(Xd.view, out=plain, beta=beta)
            assert_equal(host(out), E.colsum_ref(X, beta, out0), f"n={n} sums beta={beta}")
            R.assert_bits(host(out), host(plain), "rows_to_slots sums vs colsum")
        assert_equal(send.get(), ref, f"n={n} send buffer")
        send.assert_untouched_outside("rows_to_slots")
        if n_slots:
            assert torch.equal(send.view, ops.gather_rows(Xd.view, dev(env, send_idx)))


# ------------------------------------------------------------------------------------------------ row sums
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("C", E.ROWSUM_COLS)
def test_rowsum(env, C, pad):
    ops = env["ops"]
    n = 9       # three workgroups of four rows, the last with one
    X = E.exact_matrix(n, C, seed=2)
    assert_equal(host(ops.rowsum(Pitched(env["dev"], n, C, pad, 0, X).view)), E.rowsum_exact_ref(X), "rowsum, exact data")
    if C <= 64:     # the documented ascending order
        Xr = np.random.default_rng(C).uniform(-1, 1, (n, C)).astype(np.float32)
        R.assert_bits(host(ops.rowsum(Pitched(env["dev"], n, C, pad, 0, Xr).view)), E.rowsum_ascending_ref(Xr), "rowsum, ascending order")


# ------------------------------------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("pad", [0, 4, 1])
@pytest.mark.parametrize("F", [4, 16, 256, 1024, 7, 100, 300])
def test_gather_and_scatter_add_rows(env, F, pad):
    ops = env["ops"]
    rng = np.random.default_rng([F, pad])
    n_src = 50
    X = rng.uniform(-1, 1, (n_src, F)).astype(np.float32)
    Xd = Pitched(env["dev"], n_src, F, pad, 0, X)
    for idx in (np.array([17], dtype=np.int32), rng.integers(0, n_src, 37).astype(np.int32), np.array([3, 3, 3, 49, 0, 49], dtype=np.int32)):
        out = Pitched(env["dev"], len(idx), F, pad)
        ops.gather_rows(Xd.view, dev(env, idx), out=out.view)
        R.assert_bits(out.get(), E.gather_ref(X, idx), f"gather of {len(idx)} rows")
        out.assert_untouched_outside("gather_rows")
    # scatter-add: unique indices only (no atomics in the kernel; include/gnnx.h)
    Y = rng.uniform(-1, 1, (n_src, F)).astype(np.float32)
    for idx in (np.array([49], dtype=np.int32), rng.permutation(n_src)[:33].astype(np.int32)):
        inp = rng.uniform(-1, 1, (len(idx), F)).astype(np.float32)
        Yd = Pitched(env["dev"], n_src, F, pad, 0, Y)
        ops.scatter_add_rows(Pitched(env["dev"], len(idx), F, pad, 0, inp).view, dev(env, idx), Yd.view)
        R.assert_bits(Yd.get(), E.scatter_add_ref(Y, inp, idx), f"scatter-add of {len(idx)} rows")
        Yd.assert_untouched_outside("scatter_add_rows")


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("shape", [(1, 1), (31, 33), (32, 32), (33, 65), (1000, 3), (3, 1000), (2_097_185, 3), (3, 2_097_185)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_transpose(env, shape):
    """Y[c, r] = X[r, c] on padded pitches; the tall and the wide case have 65 537 tiles along one side (more than grid.y could hold)."""
    ops = env["ops"]
    rows, cols = shape
    X = np.random.default_rng(rows).integers(-1000, 1000, (rows, cols)).astype(np.float32)
    Xd, Yd = Pitched(env["dev"], rows, cols, 3, 0, X), Pitched(env["dev"], cols, rows, 5)
    ops.transpose(Xd.view, out=Yd.view)
    assert_equal(Yd.get(), X.T, "transpose")
    Yd.assert_untouched_outside("transpose")


# ------------------------------------------------------------------------------------------------ axpy, fill, sgd
@pytest.mark.parametrize("n", [0, 1, 255, 257, 600_001])
def test_axpy_fill_sgd(env, n):
    """y + a * x with two roundings; p - lr * (g + wd * p) with the wd * p term skipped at wd == 0; fill; n = 0 touches nothing.
    Each vector sits between sentinels."""
    ops, torch = env["ops"], env["torch"]
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)

    def guarded(a):
        buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=env["dev"])
        if n:
            buf[4:4 + n] = dev(env, a)
        return buf, buf[4:4 + n]

    def check(buf, ref, what):
        h = host(buf)
        R.assert_bits(h[4:4 + n], ref, what)
        assert (h[:4] == SENTINEL).all() and (h[4 + n:] == SENTINEL).all(), f"{what}: wrote outside its n elements"

    xd = dev(env, x)
    for a in (0.3, -1.0):
        buf, yv = guarded(y)
        ops.axpy(a, xd, yv)
        check(buf, E.axpy_ref(a, x, y), f"axpy a={a}")
    for lr, wd in ((0.01, 0.0), (0.01, 5e-4), (0.5, -0.25)):
        buf, pv = guarded(y)
        ops.sgd_step(pv, xd, lr, wd)
        check(buf, E.sgd_ref(y, x, lr, wd), f"sgd lr={lr} wd={wd}")
    for value in (1.25, -0.0, float("inf")):
        buf, v = guarded(y)
        ops.fill(v, value)
        check(buf, np.full(n, value, dtype=np.float32), f"fill {value}")
    if n >= 255:    # wd == 0 leaves an infinite parameter infinite and the sign of a zero gradient alone
        p = y.copy()
        p[:3], g = (np.inf, -np.inf, 0.0), x.copy()
        g[:3] = (1.0, -0.0, -0.0)
        buf, pv = guarded(p)
        ops.sgd_step(pv, dev(env, g), 0.1, 0.0)
        check(buf, E.sgd_ref(p, g, 0.1, 0.0), "sgd on inf / -0")


# ------------------------------------------------------------------------------------------------ f32 -> bf16
@pytest.mark.parametrize("form", ["vector", "scalar"])
def test_f32_to_bf16_special_values(env, form):
    """Ties to even in both directions, overflow to inf, +-inf, +-0, denormals: the bits of torch.bfloat16 (and of the plain
    round-to-nearest-even restatement).  A NaN stays a NaN (payload not compared).  Scalar form: destination shifted by one element."""
    ops, torch = env["ops"], env["torch"]
    u = np.concatenate([E.BF16_TABLE, E.BF16_NANS, E.BF16_TABLE[:1]])
    assert len(u) % 4 == 0
    n_fin = len(E.BF16_TABLE)
    X = dev(env, u.view(np.int32).copy()).view(torch.float32).view(len(u) // 4, 4)
    buf = torch.zeros(len(u) + 8, dtype=torch.bfloat16, device=env["dev"])
    off = 1 if form == "scalar" else 0
    out = buf[off:off + len(u)].view(len(u) // 4, 4)
    ops.to_bf16(X, out=out)
    got = host(out.view(torch.int16)).reshape(-1).view(np.uint16)
    ref = torch.from_numpy(u.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)   # on the CPU
    fin = np.r_[0:n_fin, len(u) - 1]
    assert np.array_equal(got[fin], ref[fin]), f"got {[hex(v) for v in got[fin]]}, torch {[hex(v) for v in ref[fin]]}"
    assert np.array_equal(got[:n_fin], E.bf16_rne_ref(E.BF16_TABLE))
    nan = got[n_fin:n_fin + len(E.BF16_NANS)]
    assert ((nan & 0x7F80) == 0x7F80).all() and ((nan & 0x007F) != 0).all(), f"a NaN became {[hex(v) for v in nan]}"
    assert not host(buf.view(torch.int16))[off + len(u):].any() and not host(buf.view(torch.int16))[:off].any()
