"""GPU tests of gnnx_knn_f32 / ops.knn (run with -m gpu on an MI355X) against tests/knn_ref.py: idx by equality, dist by bit pattern.

Every case runs both orders, with and without EXCLUDE_SELF.  The operands sit between NaN pads on a leading dimension above the minimum
and off the 16-byte grid; the outputs sit inside sentinel-filled buffers with ldi, ldd > k, and the WHOLE buffers are compared, so a
write behind position k - 1 or outside the rows shows.  The shapes are knn_ref.cases(): every k of {1, 2, 7, 16, 17, 63, 64}; n_feat 1
.. 5, 16, 32, the register / LDS hand-over 64 with 63 and 65, and 130; segments of 0, 1, 2, k, k + 1, 63 .. 65, both tile sizes with
one either side, 300, mixed with empty segments between full ones; m on the seams of the lane-group rule; bipartite calls with empty
query and candidate segments; identical points, +-inf and NaN coordinates.  No tolerance anywhere."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import knn_ref as kr
from tests.helpers import SENTINEL, embed

pytestmark = pytest.mark.gpu

CASES = kr.cases()
IDX_FILL = -7777
FLAGS = (0, kr.EXCLUDE_SELF, kr.NEAREST_FIRST, kr.EXCLUDE_SELF | kr.NEAREST_FIRST)
_keys = {}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def reference_keys(c):
    """The sorted key lists of a case: computed once, shared by its four flag combinations, never changed."""
    if c["name"] not in _keys:
        X, Q, sp, qp = kr.inputs(c)
        _keys[c["name"]] = kr.sorted_keys(X, Q, sp, qp)
    return _keys[c["name"]]


def place(env, a):
    """A device view of `a` between NaN pads, odd pitch, off the 16-byte grid (None for an empty matrix: no pointer to give)."""
    if a.shape[0] == 0:
        return None, a.shape[1]
    _, view = embed(env, a.shape[0], a.shape[1], "o", float("nan"))
    view.copy_(env["torch"].from_numpy(a).to(env["dev"]))
    return view, view.stride(0)


def call(env, X, Q, sp, qp, k, flags, want_dist=True):
    """gnnx_knn_f32 into sentinel-filled [m + 2, k + 3] buffers, the result at [1 : m + 1, 2 : k + 2] -> (idx buffer, dist bits buffer)."""
    torch, ops = env["torch"], env["ops"]
    n, F = X.shape
    m = n if Q is None else Q.shape[0]
    Xv, ldx = place(env, X)
    Qv, ldq = (None, 0) if Q is None else place(env, Q)
    if Q is not None and m == 0:          # a query matrix without rows has no pointer: a valid pointer that is never read
        Qv, ldq = torch.zeros((1, F), dtype=torch.float32, device=env["dev"]), F
    dsp = None if sp is None else torch.from_numpy(sp).to(env["dev"])
    dqp = None if qp is None else torch.from_numpy(qp).to(env["dev"])
    ld = k + 3
    ib = torch.full((m + 2, ld), IDX_FILL, dtype=torch.int32, device=env["dev"])
    db = torch.full((m + 2, ld), SENTINEL, dtype=torch.float32, device=env["dev"])
    iv, dv = ib[1:m + 1, 2:k + 2], db[1:m + 1, 2:k + 2]
    n_seg = 1 if sp is None else len(sp) - 1
    env["capi"].call("gnnx_knn_f32", n, m, F, n_seg, ops._ptr(Xv), ldx, ops._ptr(dsp), ops._ptr(Qv), ldq, ops._ptr(dqp), k, flags,
                     C.c_void_p(iv.data_ptr()) if m else None, ld, C.c_void_p(dv.data_ptr()) if m and want_dist else None, ld, ops._stream())
    torch.cuda.synchronize()
    return ib.cpu().numpy(), db.cpu().numpy().view(np.uint32)


def expected(m, k, idx, bits):
    ib = np.full((m + 2, k + 3), IDX_FILL, dtype=np.int32)
    db = np.full((m + 2, k + 3), SENTINEL, dtype=np.float32).view(np.uint32)
    ib[1:m + 1, 2:k + 2] = idx
    db[1:m + 1, 2:k + 2] = bits
    return ib, db


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_against_the_reference(env, c):
    X, Q, sp, qp = kr.inputs(c)
    keys, k = reference_keys(c), c["k"]
    m = len(keys)
    one = len(c["sizes"]) == 1
    first = None
    for flags in FLAGS:
        null_ptrs = one and bool(flags & kr.EXCLUDE_SELF)      # one segment: also as "both arrays NULL, n_seg == 1"
        got_i, got_d = call(env, X, Q, None if null_ptrs else sp, None if null_ptrs else qp, k, flags)
        ref_i, ref_d = expected(m, k, *kr.select(keys, k, flags))
        bad = np.nonzero((got_i != ref_i).any(1) | (got_d != ref_d).any(1))[0]
        assert bad.size == 0, (c["name"], flags, "first bad buffer row", int(bad[0]), got_i[bad[0]].tolist(), ref_i[bad[0]].tolist(),
                               got_d[bad[0]].tolist(), ref_d[bad[0]].tolist())
        if flags == 0:
            first = (got_i, got_d)
            rows = got_i[1:m + 1, 2:k + 2]
            assert ((rows[:, 1:] > rows[:, :-1]) | (rows[:, 1:] == -1)).all()       # a strictly ascending CSR row, pads behind it
    again = call(env, X, Q, sp, qp, k, 0)                                            # the same bits on a second run
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


def test_the_cases_reach_every_dispatch_cell(env):
    """From the header's rule (its constants are read from include/gnnx.h), not from a kernel name."""
    header = open(env["capi"].HEADER_PATH).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define GNNX_KNN_([A-Z_]+) (\d+)\s*$", header, flags=re.M)}
    assert (consts["REG_FEAT"], consts["TILE"], consts["TILE_LDS"], consts["FULL_LANES"], consts["GROUP_FLOATS"]) == \
        (kr.REG_FEAT, kr.TILE, kr.TILE_LDS, kr.FULL_LANES, kr.GROUP_FLOATS)
    for cell in ("{2, 3, 4, 8, 16, 32, 64}", "m * Gm >= GNNX_KNN_FULL_LANES", "Gs * 2k <= n / n_seg", "Gw * NF <= GNNX_KNN_GROUP_FLOATS",
                 "G = min(Gm, Gs, Gw)", "NF = 64 in the LDS form"):
        assert cell in header, cell
    seen = set()
    for c in CASES:
        n, m = sum(c["sizes"]), sum(c["sizes"] if c["qsizes"] is None else c["qsizes"])
        seen.add(kr.dispatch(n, m, c["n_feat"], len(c["sizes"]), c["k"]))
    assert seen >= kr.ALL_CELLS, sorted(kr.ALL_CELLS - seen, key=str)


def test_without_distances_and_through_ops(env):
    """d_dist == NULL writes indices alone; ops.knn on strided views, with and without Q, equals the raw call."""
    torch, ops = env["torch"], env["ops"]
    c = next(x for x in CASES if x["name"] == "rounded-F5-bip")
    X, Q, sp, qp = kr.inputs(c)
    keys, k, m = reference_keys(c), c["k"], Q.shape[0]
    got_i, got_d = call(env, X, Q, sp, qp, k, kr.NEAREST_FIRST, want_dist=False)
    ref_i, _ = expected(m, k, *kr.select(keys, k, kr.NEAREST_FIRST))
    assert np.array_equal(got_i, ref_i) and (got_d == np.float32(SENTINEL).view(np.uint32)).all()
    Xv, _ = place(env, X)
    Qv, _ = place(env, Q)
    dsp, dqp = torch.from_numpy(sp).to(env["dev"]), torch.from_numpy(qp).to(env["dev"])
    for nearest in (False, True):
        idx, dist = ops.knn(Xv, k, Q=Qv, segptr=dsp, qsegptr=dqp, nearest_first=nearest)
        ri, rd = kr.select(keys, k, kr.NEAREST_FIRST if nearest else 0)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (m, k)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(dist.cpu().numpy().view(np.uint32), rd)
    idx, dist = ops.knn(Xv, 3, segptr=dsp, exclude_self=True, want_dist=False)
    assert dist is None and np.array_equal(idx.cpu().numpy(), kr.knn_ref(X, 3, segptr=sp, flags=kr.EXCLUDE_SELF)[0])
    e_idx, e_dist = ops.knn(Xv, 3, Q=Qv[:0], segptr=dsp, qsegptr=torch.zeros_like(dqp))
    assert tuple(e_idx.shape) == (0, 3) and tuple(e_dist.shape) == (0, 3)
    with pytest.raises(env["capi"].GnnxError):
        ops.knn(Xv, 65)
    with pytest.raises(env["capi"].GnnxError):
        ops.knn(Xv, 3, Q=Qv, segptr=dsp)
