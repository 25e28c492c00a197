"""Shared test helpers: load the in-tree package (its directory name `gnn.cpp_amd` contains a dot, so
it is loaded by path and registered under the importable alias `gnncpp_amd`), the tolerance helper of the
parity tests, and the chunked comparison helpers of the large-offset tests (tests/test_gpu_large_offsets.py).

The chunked helpers work on torch tensors of any device and never index a tensor past CHUNK rows in one torch call: the
EXPECTED side of a comparison is always built from row slices of at most CHUNK rows, whose element offsets stay far below
2^31, so a reference does not depend on how torch itself indexes a tensor of more than 2^31 elements.

`embed` / `holds_fill` put an operand as a view inside a poisoned buffer (the contract tests of the dense products and of their fused
epilogues)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
synth = pkg.synth

RTOL = 1e-5  # north_star: "within 1e-5 relative fp32"
CHUNK = 1_000_000  # rows per reference chunk: 256 M elements of a 256-wide matrix, element offsets < 2^28
NUM_CU, TILE_ROWS = 256, 256  # gnnx_common.h kNumCU, the LDS-DMA product's main tile height


def assert_close(got, ref, what="", absum=None, exact=None):
    """|got - ref| <= RTOL * max(1, |ref|[, absum]).  absum = sum_k |term_k| per output element, passed only for
    node-dimension / hub reductions (module docstring of test_gpu_parity.py).  exact = float64 result: then also require
    the GPU to be no further from it than twice the reference's own error (plus 1e-6 of the result scale)."""
    got64, ref64 = got.astype(np.float64), ref.astype(np.float64)
    err = np.abs(got64 - ref64)
    scale = np.maximum(1.0, np.abs(ref64))
    if absum is not None:
        scale = np.maximum(scale, absum)
    worst = float((err / (RTOL * scale)).max()) if err.size else 0.0
    assert worst <= 1.0, f"{what}: max err/bound = {worst:.3f}"
    if exact is not None and err.size:
        assert_no_worse_than_reference(got, ref, exact, what)


def assert_no_worse_than_reference(got, ref, exact, what=""):
    """The `exact=` clause of assert_close on its own, for a node-dimension reduction whose reference (the oracle's sequential f32 sum) is
    itself further than 1e-5 from float64: the GPU must be no further from the float64 result than twice the reference's own error
    (plus 1e-6 of the result scale)."""
    e_gpu = np.abs(got.astype(np.float64) - exact).max()
    e_ref = np.abs(ref.astype(np.float64) - exact).max()
    assert e_gpu <= 2.0 * e_ref + 1e-6 * max(1.0, np.abs(exact).max()), \
        f"{what}: GPU error vs float64 {e_gpu:.3e} exceeds reference's own {e_ref:.3e}"


# ------------------------------------------------------------------ tall matrices, chunk by chunk
def row_chunks(n, step=CHUNK):
    """(r0, r1) row ranges of at most `step` rows covering 0..n."""
    for r0 in range(0, int(n), step):
        yield r0, min(int(n), r0 + step)


def fill_small_ints(t, gen, lo=-1, hi=1, step=CHUNK):
    """Fill the 2-D tensor (or strided view) `t` in place, row chunk by row chunk, with integers drawn uniformly from lo..hi
    (stored in t's dtype) from the one seeded generator `gen`.  With entries in {-1, 0, 1} every product is an integer and every
    partial sum over n <= 2^24 rows is an integer below 2^24 in magnitude: exact in f32 in ANY summation order."""
    for r0, r1 in row_chunks(t.shape[0], step):
        t[r0:r1].random_(lo, hi + 1, generator=gen)
    return t


def dma_tail_round(M):
    """r of the tall product's tile plan (gnnx_gemm.hip launch_dma): the number of 256-row tiles left after the whole rounds of one
    tile per CU.  1..64: the last round runs on 128 x 128 tiles, 65..128: on 256 x 128 tiles, else no launch of its own."""
    return (int(M) // TILE_ROWS) % NUM_CU


def sample_rows(M, seed=0):
    """Ascending unique rows of an M-row matrix that a CPU reference checks when it cannot check all: rows 0..599; 8 388 300 ..
    8 388 900 (the element offset of a 256-wide row passes 2^31 at row 8 388 608); the first and last row of every 1000th 256-row
    tile; the last full round of 256 tiles; the last 700 rows; 3000 seeded random rows."""
    M = int(M)
    mt = M // TILE_ROWS
    r = mt % NUM_CU
    parts = [np.arange(0, min(600, M)), np.arange(min(8_388_300, M), min(8_388_901, M))]
    t0 = np.arange(0, -(-M // TILE_ROWS), 1000, dtype=np.int64) * TILE_ROWS
    parts += [t0, np.minimum(t0 + TILE_ROWS - 1, M - 1)]
    if mt - r >= NUM_CU:
        parts.append(np.arange((mt - r - NUM_CU) * TILE_ROWS, (mt - r) * TILE_ROWS))
    parts.append(np.arange(max(0, M - 700), M))
    parts.append(np.random.default_rng(seed).integers(0, M, 3000))
    return np.unique(np.concatenate([p.astype(np.int64) for p in parts]))


def take_rows(T, rows, step=CHUNK):
    """T[rows] (rows ascending, numpy int64) as a host numpy array, taken chunk by chunk with torch indexing."""
    import torch
    rows = np.asarray(rows, dtype=np.int64)
    out = []
    for r0, r1 in row_chunks(T.shape[0], step):
        sel = rows[(rows >= r0) & (rows < r1)]
        if sel.size:
            out.append(T[r0:r1][torch.from_numpy(sel - r0).to(T.device)].cpu())
    return torch.cat(out).numpy() if out else np.zeros((0,) + tuple(T.shape[1:]), dtype=np.float32)


def _describe_rows(bad_rows, n_bad_elements):
    first, last = int(bad_rows[0]), int(bad_rows[-1])
    return (f"{n_bad_elements} elements in {len(bad_rows)} rows differ; first row {first} (row % 256 = {first % 256}, tile % 256 = "
            f"{first // 256 % 256}), last row {last} (row % 256 = {last % 256}, tile % 256 = {last // 256 % 256})")


def rows_mismatch(got, ref_fn, step=CHUNK, rtol=None, absum_fn=None, atol=None, ref_scale=None):
    """Compare got[r0:r1] with ref_fn(r0, r1) (float64, same shape; or a pair (reference, bool mask of the elements that count)) for
    every row chunk.  rtol and atol None: every element must be EQUAL (the exact legs; a NaN differs).  atol: |got - ref| <= atol.
    rtol: |got - ref| <= rtol * max(1, |ref|[, absum_fn(r0, r1)]), or rtol * ref_scale when one scale holds for the whole matrix.
    Returns None when every row passes, else a description: count, first and last failing row and where they sit in their tile
    and CU round."""
    import torch
    bad, n_el, worst = [], 0, 0.0
    for r0, r1 in row_chunks(got.shape[0], step):
        ref = ref_fn(r0, r1)
        keep = None
        if isinstance(ref, tuple):
            ref, keep = ref
        g = got[r0:r1].double()
        assert g.shape == ref.shape, f"reference chunk has shape {tuple(ref.shape)}, rows {r0}:{r1} have {tuple(g.shape)}"
        if rtol is None and atol is None:
            ne = g != ref
        else:
            if atol is not None:
                bound = atol
            elif ref_scale is not None:
                bound = rtol * ref_scale
            else:
                scale = ref.abs().clamp_min(1.0)
                if absum_fn is not None:
                    scale = torch.maximum(scale, absum_fn(r0, r1))
                bound = rtol * scale
            ratio = (g - ref).abs() / bound
            if keep is not None:
                ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
            ne = ~(ratio <= 1.0)        # a NaN fails
            if ratio.numel():
                worst = max(worst, float(ratio.nan_to_num(nan=float("inf")).max()))
        if keep is not None:
            ne = ne & keep
        if bool(ne.any()):
            n_el += int(ne.sum())
            ne = ne.reshape(ne.shape[0], -1).any(1)
            bad.append((ne.nonzero().flatten() + r0).cpu())
    if not bad:
        return None
    msg = _describe_rows(torch.cat(bad).numpy(), n_el)
    return msg if rtol is None and atol is None else msg + f"; worst err/bound = {worst:.3f}"


def assert_rows_equal(got, ref_fn, what, step=CHUNK):
    """The exact leg: every element of every row equals the float64 reference built chunk by chunk."""
    msg = rows_mismatch(got, ref_fn, step)
    assert msg is None, f"{what}: {msg}"


def assert_rows_close(got, ref_fn, what, rtol=RTOL, absum_fn=None, atol=None, ref_scale=None, step=CHUNK):
    """The rounding leg over ALL rows: |got - ref| <= rtol * max(1, |ref|[, absum]) (or atol, or rtol * ref_scale) against float64
    chunks."""
    msg = rows_mismatch(got, ref_fn, step, rtol=rtol if atol is None else None, absum_fn=absum_fn, atol=atol, ref_scale=ref_scale)
    assert msg is None, f"{what}: {msg}"


def assert_small_equal(got, ref64, what):
    """Exact leg of a reduction's small output ([F], [F, F]): got == ref64 everywhere (the dropped-row detector)."""
    g = got.double().reshape(-1, got.shape[-1])
    assert_rows_equal(g, lambda r0, r1: ref64.reshape(-1, ref64.shape[-1])[r0:r1], what)


def chunked_sum(fn, n, step=CHUNK):
    """sum over row chunks of fn(r0, r1) (float64 tensors of one shape): the float64 reference of a node-dimension reduction."""
    acc = None
    for r0, r1 in row_chunks(n, step):
        v = fn(r0, r1)
        acc = v if acc is None else acc + v
    return acc


# ------------------------------------------------------------------ outputs between sentinels
SENTINEL = -12345.0


class Pitched:
    """An [n, F] float32 device view on the leading dimension F + pad, `off` elements into its buffer, with two rows behind it;
    everything that is not the view holds SENTINEL.  data None: the view holds the sentinel too (an output).  The checks run on the
    device: the buffers can be large."""

    def __init__(self, device, n, F, pad=0, off=0, data=None):
        import torch
        self.n, self.F, self.ld, self.off = n, F, F + pad, off
        self.buf = torch.full((off + (n + 2) * self.ld,), SENTINEL, dtype=torch.float32, device=device)
        self.view = self.buf[off:].view(n + 2, self.ld)[:n, :F]
        if data is not None and n:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(device))

    def get(self):
        return self.view.detach().cpu().numpy()

    def assert_untouched_outside(self, what):
        body = self.buf[self.off:].view(self.n + 2, self.ld)
        ok = (self.buf[:self.off] == SENTINEL).all() & (body[:self.n, self.F:] == SENTINEL).all() & (body[self.n:] == SENTINEL).all()
        assert bool(ok), f"{what}: wrote outside its [n, F] elements"

    def assert_untouched(self, what):
        assert bool((self.buf == SENTINEL).all()), f"{what}: the output was written"


# ------------------------------------------------------------------ operands inside poisoned buffers
ROWS_BEFORE, ROWS_AFTER = 3, 2


def embed(env, rows, cols, mode, fill):
    """(buffer, view): a [rows, cols] view inside a buffer full of `fill`.  mode "a": column offset 4, pitch a multiple of 4 (the view
    starts on the 16-byte grid); "o": odd pitch and a first element off the grid (column offset 1, or 2 where 1 would land on it): ld % 4 != 0 and a misaligned
    base, the two conditions that switch every vector access off."""
    torch = env["torch"]
    if mode == "a":
        left, pitch = 4, (cols + 8 + 3) // 4 * 4
    else:
        pitch = cols + 3 + (cols % 2)
        left = 1 if (ROWS_BEFORE * pitch + 1) % 4 else 2         # the first element off the 16-byte grid as well as the pitch
    buf = torch.full((rows + ROWS_BEFORE + ROWS_AFTER, pitch), fill, dtype=torch.float32, device=env["dev"])
    view = buf[ROWS_BEFORE:ROWS_BEFORE + rows, left:left + cols]
    assert pitch > cols + left and view.stride(0) == pitch
    assert (pitch % 4 == 0) == (mode == "a")
    if view.numel():
        assert (view.data_ptr() % 16 == 0) == (mode == "a")
    return buf, view


def holds_fill(buf, fill):
    return bool(buf.isnan().all()) if fill != fill else bool((buf == fill).all())
