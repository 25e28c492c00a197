"""GPU tests of the opt-in split-precision product gnnx_gemm_split_bf16_f32 (gnn.cpp_amd/csrc/gnnx_gemm_split.hip; run with -m gpu on
an MI355X) against tests/gemm_split_ref.py.

Which path a shape reaches (128 x 64 NB output tile, K step 16, two LDS buffers):

  N = 128: NB = 2, one workgroup per 128 rows; 256: NB = 4 (a second B granule per thread), one; 384: NB = 2, three; 512: NB = 4, two.
  K = 16: the prologue's tile only, the loop never loads; 32 / 48: an even / odd tile count (the last tile in either LDS buffer).
  M = 1, 127, 128, 129, 300: the loader clamps rows past M onto row M - 1; those lanes compute and must not store.

Exact families (integers: every piece product and every partial sum is exact, so the result must EQUAL the integer product -- one
family per group of the six kept piece products), operands and C on padded leading dimensions between NaN and sentinels, general
data against float64 within the f32 chain's worst case K 2^-24 |A||B|, power-of-two scales bit for bit, non-finite operands that
stay in their row or column, every refusal by its status, and the bench.py --split-gemm leg."""
import ctypes as C
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

from tests import gemm_split_ref as S
from tests import norm_ref as R
from tests.helpers import ROOT, SENTINEL          # (tests.helpers also registers the in-tree package)

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


def in_nan(env, X, pad):
    """X as the first columns of a NaN-filled buffer with `pad` more columns (pad 0: X itself, contiguous)."""
    torch = env["torch"]
    buf = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), dtype=torch.float32, device=env["dev"])
    buf[:, :X.shape[1]] = dev(env, X)
    view = buf[:, :X.shape[1]]
    assert view.stride(0) == X.shape[1] + pad and view.data_ptr() % 16 == 0
    return view


def b_operand(env, B, transB, pad=0):
    """B [N, K] as the call's operand: itself (transB) or its transpose (k-major), the leading dimension `pad` above the minimum."""
    return in_nan(env, B if transB else B.T, pad)


def split(env, A, B, transB, lda_pad=0, ldb_pad=0):
    """ops.gemm_split on host operands A [M, K], B [N, K]; returns the host result."""
    return host(env["ops"].gemm_split(in_nan(env, A, lda_pad), b_operand(env, B, transB, ldb_pad), transB=transB))


@functools.lru_cache(maxsize=4)
def family(name, M, N, K):
    """One draw per case, shared by the contiguous and the padded test that follow each other."""
    return S.exact_family(name, M, N, K)


LAYOUTS = ((True, "B [N, K]"), (False, "B k-major"))


# ------------------------------------------------------------------------------------------------ exact families
@pytest.mark.parametrize("M,N,K", S.EXACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", S.FAMILIES)
def test_exact_family_equals_integer_product(env, name, M, N, K):
    """Equality with the int64 product on every element, in both layouts of B (which then hold the same bits)."""
    A, B, ref = family(name, M, N, K)
    for transB, what in LAYOUTS:
        got = split(env, A, B, transB)
        assert np.array_equal(got, ref), f"family {name}, M={M} N={N} K={K}, {what}: {R.describe_mismatch(got, ref)}"


@pytest.mark.parametrize("M,N,K", S.EXACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", S.FAMILIES)
def test_exact_family_on_padded_leading_dimensions(env, name, M, N, K):
    """lda = K + 4 and K + 12, ldb 4 above its minimum (NaN in every pad element), C the first N columns and M rows of an
    (M + 3) x (N + 4) buffer of sentinels: the same equality, and nothing written outside the M x N block."""
    ops, torch = env["ops"], env["torch"]
    A, B, ref = family(name, M, N, K)
    for transB, what in LAYOUTS:
        for lda_pad in (4, 12):
            where = f"family {name}, M={M} N={N} K={K}, lda=K+{lda_pad}, {what} ldb=min+4, ldc=N+4"
            buf = torch.full((M + 3, N + 4), SENTINEL, dtype=torch.float32, device=env["dev"])
            ops.gemm_split(in_nan(env, A, lda_pad), b_operand(env, B, transB, 4), transB=transB, out=buf[:M, :N])
            got = host(buf)
            assert np.array_equal(got[:M, :N], ref), f"{where}: {R.describe_mismatch(got[:M, :N], ref)}"
            got[:M, :N] = SENTINEL
            assert (got == SENTINEL).all(), f"{where}: wrote outside the M x N block, first at {tuple(np.argwhere(got != SENTINEL)[0])}"


@pytest.mark.parametrize("name", S.FAMILIES)
def test_exact_family_with_b_and_c_off_the_16_byte_grid(env, name):
    """Only A has to be 16-byte aligned with lda % 4 == 0: B and C one float off the grid on odd leading dimensions."""
    ops, torch = env["ops"], env["torch"]
    M, N, K = 129, 256, 32
    A, B, ref = family(name, M, N, K)
    for transB, what in LAYOUTS:
        Bh = B if transB else B.T
        bbuf = torch.full((Bh.shape[0], Bh.shape[1] + 3), float("nan"), dtype=torch.float32, device=env["dev"])
        bview = bbuf[:, 1:1 + Bh.shape[1]]
        bview.copy_(dev(env, Bh))
        cbuf = torch.full((M + 3, N + 3), SENTINEL, dtype=torch.float32, device=env["dev"])
        assert bview.data_ptr() % 16 == 4 and bview.stride(0) % 2 == 1 and cbuf[:M, 1:N + 1].data_ptr() % 16 == 4
        ops.gemm_split(in_nan(env, A, 4), bview, transB=transB, out=cbuf[:M, 1:N + 1])
        got = host(cbuf)
        where = f"family {name}, M={M} N={N} K={K}, {what}, B and C misaligned"
        assert np.array_equal(got[:M, 1:N + 1], ref), f"{where}: {R.describe_mismatch(got[:M, 1:N + 1], ref)}"
        got[:M, 1:N + 1] = SENTINEL
        assert (got == SENTINEL).all(), f"{where}: wrote outside the M x N block"


# ------------------------------------------------------------------------------------------------ general data against float64
@pytest.mark.parametrize("M,N,K", S.GENERAL_SHAPES, ids=lambda v: str(v))
def test_general_data_within_the_f32_chain_bound(env, M, N, K):
    """|C - A.B^T (float64)| <= K 2^-24 |A|.|B|^T on every element: the worst case of an f32 chain of K roundings.  (The kernel has
    6 K / 16 accumulating MFMA instructions and three dropped terms of at most 2^-24 each; with two roundings an instruction that is
    12 K / 16 + 3 <= K from K = 16 up.)  Prints the worst err / (2^-24 absum); both layouts of B give the same bits."""
    A, B = S.general_pair(M, N, K)
    got = split(env, A, B, True)
    R.assert_bits(split(env, A, B, False), got, f"M={M} N={N} K={K}: k-major B against B [N, K]")
    err, unit = np.abs(got.astype(np.float64) - S.product64(A, B)), S.U24 * S.absum(A, B)
    assert (unit > 0).all()
    ratio = err / unit
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"\ngemm_split general data M={M} N={N} K={K}: worst err / (2^-24 absum) = {ratio.max():.4f} at {tuple(int(v) for v in at)} "
          f"(bound K = {K}); rms = {np.sqrt((ratio ** 2).mean()):.4f}")
    assert (ratio <= K).all(), f"M={M} N={N} K={K}: worst err / (2^-24 absum) = {ratio.max():.3f} > K at {tuple(int(v) for v in at)}"


# ------------------------------------------------------------------------------------------------ scale
def test_power_of_two_scales_commute_bit_for_bit(env):
    """gemm_split(A 2^p, B 2^q) == ldexp(gemm_split(A, B), p + q): no fixed threshold and no flush anywhere in the split."""
    M, N, K = S.SCALE_SHAPE
    A, B = S.general_pair(M, N, K)
    for transB, what in LAYOUTS:
        plain = split(env, A, B, transB)
        assert np.isfinite(plain).all() and plain.any()
        for p, q in S.SCALES:
            S.check_scale(A, B, p, q)
            ref = np.ldexp(plain, p + q).astype(np.float32)
            assert np.array_equal(ref.astype(np.float64), plain.astype(np.float64) * 2.0 ** (p + q))
            R.assert_bits(split(env, S.scaled(A, p), S.scaled(B, q), transB), ref, f"scales 2^{p}, 2^{q}, {what}")


# ------------------------------------------------------------------------------------------------ non-finite operands
def assert_poisoned(got, clean, rows, cols, what):
    """Rows `rows` and columns `cols` of got hold no finite value; every other element has the bits of `clean`."""
    hit = np.zeros(got.shape, dtype=bool)
    hit[list(rows), :] = True
    hit[:, list(cols)] = True
    assert not np.isfinite(got[hit]).any(), f"{what}: {int(np.isfinite(got[hit]).sum())} finite elements in a poisoned row or column"
    assert np.isfinite(clean).all()
    rest = np.where(hit, clean, got)
    assert np.isfinite(rest).all(), f"{what}: non-finite values left their row or column, first at {tuple(np.argwhere(~np.isfinite(rest))[0])}"
    R.assert_bits(rest, clean, f"{what}: elements outside the poisoned rows and columns")


def test_nonfinite_operands_stay_in_their_row_or_column(env):
    """An Inf or NaN of A poisons its row of C, one of B its column, and nothing else changes by a bit -- with the Inf in row
    M - 1, the row the loader's clamp hands to every lane past M."""
    M, N, K = S.NONFINITE_SHAPE
    A, B = S.general((1, "x"), (M, K)), S.general((1, "w"), (N, K), scale=0.25)
    A_bad, A_zero = A.copy(), A.copy()
    A_bad[M - 1, 3], A_bad[5, 20] = np.inf, np.nan
    A_zero[M - 1, 3] = A_zero[5, 20] = 0.0
    B_bad, B_zero = B.copy(), B.copy()
    B_bad[7, 9], B_zero[7, 9] = -np.inf, 0.0
    for transB, what in LAYOUTS:
        assert_poisoned(split(env, A_bad, B, transB), split(env, A_zero, B, transB), (M - 1, 5), (), f"+Inf and NaN in A, {what}")
        assert_poisoned(split(env, A, B_bad, transB), split(env, A, B_zero, transB), (), (7,), f"-Inf in B, {what}")


# ------------------------------------------------------------------------------------------------ refusals and the empty product
class Call:
    """The arguments of one valid call (M = 100, N = 128, K = 16) on buffers with room to spare, C full of sentinels; status() makes the
    call with some of them replaced and returns the status."""

    def __init__(self, env, transB=1):
        torch = env["torch"]
        self.env, self.M, self.N, self.K = env, 100, 128, 16
        self.A = torch.ones((self.M, 64), dtype=torch.float32, device=env["dev"])
        self.B = torch.ones((128, 192), dtype=torch.float32, device=env["dev"])
        self.Cbuf = torch.full((self.M, 192), SENTINEL, dtype=torch.float32, device=env["dev"])
        need = C.c_size_t(0)
        env["capi"].call("gnnx_gemm_split_workspace", self.M, self.N, self.K, C.byref(need))
        assert need.value == 2 * 3 * self.N * self.K
        self.ws = torch.zeros(4 * need.value, dtype=torch.uint8, device=env["dev"])
        self.args = dict(transB=transB, M=self.M, N=self.N, K=self.K, A=self.A.data_ptr(), lda=self.K, B=self.B.data_ptr(),
                         ldb=self.K if transB else self.N, C=self.Cbuf.data_ptr(), ldc=self.N, ws=self.ws.data_ptr(), ws_bytes=need.value)
        assert self.A.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0

    def need(self, M, N, K):
        n = C.c_size_t(0)
        self.env["capi"].call("gnnx_gemm_split_workspace", M, N, K, C.byref(n))
        return n.value

    def status(self, **change):
        a = dict(self.args, **change)
        capi, torch = self.env["capi"], self.env["torch"]
        try:
            capi.call("gnnx_gemm_split_bf16_f32", a["transB"], a["M"], a["N"], a["K"], a["A"], a["lda"], a["B"], a["ldb"], a["C"], a["ldc"],
                      a["ws"], a["ws_bytes"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
            st = 0
        except capi.GnnxError as e:
            st = e.status
        torch.cuda.synchronize()
        return st

    def untouched(self):
        return bool((self.Cbuf == SENTINEL).all())


INVALID_ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -4, -7


@pytest.mark.parametrize("transB", (1, 0))
def test_refusals_by_status_and_c_untouched(env, transB):
    c = Call(env, transB)
    ld_k = (lambda K: K) if transB else (lambda K: c.N)
    cases = [
        ("K = 40", dict(K=40, lda=40, ldb=ld_k(40), ws_bytes=c.need(c.M, c.N, 40)), UNSUPPORTED),
        ("N = 100", dict(N=100, ldb=c.K if transB else 100, ldc=100, ws_bytes=c.need(c.M, 100, c.K)), UNSUPPORTED),
        ("K = 0", dict(K=0, lda=4, ldb=ld_k(4)), UNSUPPORTED),
        ("A one float off the 16-byte grid", dict(A=c.args["A"] + 4), UNSUPPORTED),
        ("A 8 bytes off the 16-byte grid", dict(A=c.args["A"] + 8), UNSUPPORTED),
        ("lda = K + 2", dict(lda=c.K + 2), UNSUPPORTED),
        ("lda = K - 4", dict(lda=c.K - 4), UNSUPPORTED),
        ("workspace one byte short", dict(ws_bytes=c.args["ws_bytes"] - 1), WORKSPACE),
        ("workspace 8 bytes off the 16-byte grid", dict(ws=c.args["ws"] + 8), WORKSPACE),
        ("no workspace", dict(ws=None), WORKSPACE),
        ("ldb one below its minimum", dict(ldb=c.args["ldb"] - 1), SHAPE),
        ("ldc = N - 1", dict(ldc=c.N - 1), SHAPE),
        ("M < 0", dict(M=-1), INVALID_ARG),
        ("N < 0", dict(N=-128), INVALID_ARG),
        ("K < 0", dict(K=-16), INVALID_ARG),
        ("no A", dict(A=None), INVALID_ARG),
        ("no B", dict(B=None), INVALID_ARG),
        ("no C", dict(C=None), INVALID_ARG),
    ]
    for what, change, expected in cases:
        assert c.status(**change) == expected, f"{what} (transB={transB}): status {c.status(**change)}, expected {expected}"
        assert c.untouched(), f"{what} (transB={transB}): C was written by a refused call"
    # the empty products are no error and touch nothing, with or without operands
    for what, change in (("M = 0", dict(M=0)), ("N = 0", dict(N=0, ldc=4)), ("M = 0 and N = 0", dict(M=0, N=0))):
        for nulls in (dict(), dict(A=None, B=None, ws=None, ws_bytes=0), dict(A=None, B=None, C=None, ws=None, ws_bytes=0)):
            assert c.status(**dict(change, **nulls)) == 0, f"{what} (transB={transB}, {sorted(nulls)}): not OK"
            assert c.untouched(), f"{what} (transB={transB}): C was written by an empty product"
    # and the call the cases were derived from is a valid one: ones . ones = K
    assert c.status() == 0
    flat = host(c.Cbuf).reshape(-1)
    assert (flat[:c.M * c.N] == c.K).all(), "the valid call: ones . ones != K"
    assert (flat[c.M * c.N:] == SENTINEL).all(), "the valid call wrote past its M x N elements (ldc = N)"


# ------------------------------------------------------------------------------------------------ the bench leg
def test_bench_split_gemm_leg_within_the_bound(env):
    """bench.py's step with split_gemm set against the plain step on the same runner (F = 128): dH, dW and dbias take no split
    product and hold the same bits; H = X.W^T and dX = dH.W differ by at most twice the f32 chain bound (either side carries an
    error against float64), and out by at most the aggregation of H's bound."""
    import oracle
    torch, ops, capi = env["torch"], env["ops"], env["capi"]
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    pkg = bench.load_package()
    n, F = 3000, 128
    r = bench.SingleGpu(ops, capi, pkg, env["dev"], n, 10 * n, F, None, 7, 1024)
    assert r.Fp == F
    keys = ("H", "out", "dH", "dX", "dW", "dbias")
    runs = {}
    for split_gemm in (False, True):
        r.split_gemm = split_gemm
        r.step()
        torch.cuda.synchronize()
        runs[split_gemm] = {k: host(getattr(r, k)).copy() for k in keys}
    plain, got = runs[False], runs[True]
    for k in ("dH", "dW", "dbias"):
        R.assert_bits(got[k], plain[k], f"--split-gemm: {k} takes no split product")
    X, W = host(r.X), host(r.W)
    bound_H = 2.0 * S.error_bound(X, W)                                  # H = X . W^T
    bound_dX = 2.0 * S.error_bound(plain["dH"], W.T)                     # dX = dH . W: B [N, K] is W^T
    for k, bound in (("H", bound_H), ("dX", bound_dX)):
        err = np.abs(got[k].astype(np.float64) - plain[k].astype(np.float64))
        assert (err <= bound).all(), f"--split-gemm: {k} off by {float((err / bound).max()):.3f} of twice the f32 chain bound"
        assert err.any(), f"--split-gemm: {k} has the plain product's bits -- did the split product run?"
        # and each side on its own against float64
        exact = S.product64(X, W) if k == "H" else S.product64(plain["dH"], W.T)
        for name, run in (("split", got), ("plain", plain)):
            assert (np.abs(run[k].astype(np.float64) - exact) <= bound / 2).all(), f"{name} {k} against float64"
    g = r.g
    bound_out = oracle.aggregate_fwd(host(g.rowptr), host(g.colidx), bound_H.astype(np.float32), host(g.norm), None).astype(np.float64)
    err = np.abs(got["out"].astype(np.float64) - plain["out"].astype(np.float64))
    assert (err <= bound_out).all(), f"--split-gemm: out off by {float((err / np.maximum(bound_out, 1e-300)).max()):.3f} of the aggregated bound"
