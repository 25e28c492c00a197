"""CPU tests of the nearest-neighbour call (no GPU needed): the reference restatement tests/knn_ref.py against hand-written literals; that
a wrongly associated distance chain is visible in the bits; the header, the exports and the argument validation of gnnx_knn_f32, which
happens before any device call; the Python surface; and that the shapes of tests/test_gpu_knn.py reach every cell of the dispatch."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from tests import knn_ref as kr
from tests.helpers import ROOT

NAN, INF = float("nan"), float("inf")
QNAN, PINF = kr.QNAN, kr.INF


def f32(rows):
    return np.array(rows, dtype=np.float32)


def bits(rows):
    return np.array(rows, dtype=np.float32).view(np.uint32)


def test_row_of_points_with_ties():
    X = f32([[0], [1], [2], [3], [5]])
    idx, d = kr.knn_ref(X, 2, flags=kr.EXCLUDE_SELF)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 3], [1, 2], [2, 3]]       # point 3: rows 1 and 4 tie at 4, the smaller row wins
    assert np.array_equal(d, bits([[1, 4], [1, 1], [1, 1], [4, 1], [9, 4]]))
    idx, d = kr.knn_ref(X, 2, flags=kr.EXCLUDE_SELF | kr.NEAREST_FIRST)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 3], [2, 1], [3, 2]]       # equal distances: the smaller row first
    assert np.array_equal(d, bits([[1, 4], [1, 1], [1, 1], [1, 4], [4, 9]]))
    idx, _ = kr.knn_ref(X, 1, flags=kr.EXCLUDE_SELF)
    assert idx.tolist() == [[1], [0], [1], [2], [3]]
    idx, d = kr.knn_ref(X, 1)                                              # with itself allowed every point is its own nearest
    assert idx.tolist() == [[0], [1], [2], [3], [4]] and not d.any()


def test_nan_coordinate_comes_last():
    X = f32([[0], [NAN], [1]])
    idx, d = kr.knn_ref(X, 3, flags=kr.NEAREST_FIRST)
    assert idx.tolist() == [[0, 2, 1], [0, 1, 2], [2, 0, 1]]             # a NaN query: every distance NaN, row order
    assert d.tolist() == [[0, bits([1])[0], QNAN], [QNAN] * 3, [0, bits([1])[0], QNAN]]
    idx, d = kr.knn_ref(X, 3)
    assert idx.tolist() == [[0, 1, 2]] * 3
    assert d.tolist() == [[0, QNAN, bits([1])[0]], [QNAN] * 3, [bits([1])[0], QNAN, 0]]
    idx, _ = kr.knn_ref(X, 1, flags=kr.EXCLUDE_SELF)
    assert idx.tolist() == [[2], [0], [0]]
    # inf - inf is a NaN too, and an infinite distance sorts below it
    idx, d = kr.knn_ref(f32([[INF], [0], [INF]]), 2, flags=kr.EXCLUDE_SELF | kr.NEAREST_FIRST)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0]] and d.tolist() == [[PINF, QNAN], [PINF, PINF], [PINF, QNAN]]


def test_duplicate_point():
    X = f32([[1, 1], [1, 1], [0, 0]])
    idx, d = kr.knn_ref(X, 1, flags=kr.EXCLUDE_SELF)
    assert idx.tolist() == [[1], [0], [0]] and np.array_equal(d, bits([[0], [0], [2]]))
    idx, d = kr.knn_ref(X, 2, flags=kr.NEAREST_FIRST)
    assert idx.tolist() == [[0, 1], [0, 1], [2, 0]] and np.array_equal(d, bits([[0, 0], [0, 0], [0, 2]]))


def test_segments_shorter_than_k_and_bipartite_calls():
    X = f32([[0], [3], [10], [11], [13]])
    ptr = [0, 2, 2, 5]
    idx, d = kr.knn_ref(X, 3, segptr=ptr, flags=kr.EXCLUDE_SELF)
    assert idx.tolist() == [[1, -1, -1], [0, -1, -1], [3, 4, -1], [2, 4, -1], [2, 3, -1]]
    assert d.tolist() == [[bits([9])[0], PINF, PINF]] * 2 + [list(bits([1, 9])) + [PINF], list(bits([1, 4])) + [PINF],
                                                              list(bits([9, 4])) + [PINF]]
    idx, _ = kr.knn_ref(X, 3, segptr=ptr)
    assert idx.tolist() == [[0, 1, -1], [0, 1, -1], [2, 3, 4], [2, 3, 4], [2, 3, 4]]
    # queries of their own: segment 0 has no query, segment 1 no candidate; EXCLUDE_SELF compares ROW NUMBERS
    Q = f32([[12], [2], [2]])
    idx, d = kr.knn_ref(X, 2, Q=Q, segptr=[0, 2, 2, 5], qsegptr=[0, 0, 1, 3], flags=kr.NEAREST_FIRST)
    assert idx.tolist() == [[-1, -1], [2, 3], [2, 3]] and d[0].tolist() == [PINF, PINF]
    idx, _ = kr.knn_ref(X, 2, Q=Q, segptr=[0, 2, 2, 5], qsegptr=[0, 0, 1, 3], flags=kr.NEAREST_FIRST | kr.EXCLUDE_SELF)
    assert idx.tolist() == [[-1, -1], [2, 3], [3, 4]]                     # query row 2 loses candidate row 2; query row 1 nothing


def test_a_wrong_chain_shows_in_the_bits():
    X, Q = kr.rounded_points(5, 200, 16), kr.rounded_points(6, 50, 16)
    ref = kr.distances(Q, X).view(np.uint32)
    for wrong in (kr.distances_fma, kr.distances_f64):
        got = wrong(Q, X).view(np.uint32)
        assert (got != ref).mean() > 0.05, wrong.__name__
        assert not np.array_equal(kr.knn_ref(X, 8, Q=Q, dist_fn=wrong)[1], kr.knn_ref(X, 8, Q=Q)[1])
    # on the exact family every chain gives the same integers
    Xe, Qe = kr.exact_points(5, 200, 16), kr.exact_points(6, 50, 16)
    assert np.array_equal(kr.distances_fma(Qe, Xe), kr.distances(Qe, Xe)) and np.array_equal(kr.distances_f64(Qe, Xe), kr.distances(Qe, Xe))
    assert float(kr.distances(Qe, Xe).max()) <= 16 * 16 * 16


def test_the_gpu_shapes_reach_every_dispatch_cell():
    seen = set()
    for c in kr.cases():
        n, m = sum(c["sizes"]), sum(c["sizes"] if c["qsizes"] is None else c["qsizes"])
        seen.add(kr.dispatch(n, m, c["n_feat"], len(c["sizes"]), c["k"]))
    assert seen >= kr.ALL_CELLS, sorted(kr.ALL_CELLS - seen, key=str)
    seams = {c["qsizes"][0]: kr.dispatch(c["sizes"][0], c["qsizes"][0], 2, 1, 1)[1] for c in kr.cases() if c["name"].startswith("seam-")}
    F = kr.FULL_LANES
    assert seams == {F: 1, F - 1: 2, F // 2: 2, F // 2 - 1: 4, F // 4: 4, F // 4 - 1: 8}     # the rule by m binds on either side
    assert kr.dispatch(32768, 32768, 3, 32, 20) == (3, 8) and kr.dispatch(131072, 131072, 3, 1, 16) == (3, 2)
    assert kr.dispatch(1000, 1000, 130, 1, 4) == ("lds", 2) and kr.dispatch(10, 1 << 20, 64, 1, 1) == (64, 1)
    assert kr.dispatch(32768, 32768, 64, 32, 20) == (64, 2) and kr.dispatch(1000, 1000, 3, 1, 1) == (3, 32)      # wide rows cap the group
    assert len(kr.ALL_CELLS) == 7 + 6 + 6 + 5 + 4 + 3 + 2 + 2


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_header_constants_signature_and_exports(capi):
    L = capi.lib()
    assert "gnnx_knn_f32" in capi.declared_symbols() and hasattr(L, "gnnx_knn_f32")
    assert len(capi._SIGS["gnnx_knn_f32"]) == 17
    assert not [s for s in capi.declared_symbols() if "knn" in s and s != "gnnx_knn_f32"]      # no workspace query
    header = open(capi.HEADER_PATH).read()
    consts = {k: int(v.rstrip("u")) for k, v in re.findall(r"^#define (GNNX_KNN_[A-Z_]+) (\d+u?)\s*$", header, flags=re.M)}
    assert consts == dict(GNNX_KNN_MAX_K=kr.MAX_K, GNNX_KNN_EXCLUDE_SELF=kr.EXCLUDE_SELF, GNNX_KNN_NEAREST_FIRST=kr.NEAREST_FIRST,
                          GNNX_KNN_REG_FEAT=kr.REG_FEAT, GNNX_KNN_TILE=kr.TILE, GNNX_KNN_TILE_LDS=kr.TILE_LDS,
                          GNNX_KNN_FULL_LANES=kr.FULL_LANES, GNNX_KNN_GROUP_FLOATS=kr.GROUP_FLOATS)
    assert "tests/knn_ref.py" in header
    csrc = os.path.join(ROOT, "gnn.cpp_amd", "csrc")
    assert "gnnx_knn.hip" in open(os.path.join(csrc, "Makefile")).read()
    unit = open(os.path.join(csrc, "gnnx_knn.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and not re.search(r"atomic[A-Z_]\w*\s*\(", unit)     # atomicAdd(, atomic_fetch_add(


def test_argument_validation_without_device(capi):
    """Validation happens before any HIP call, so these return statuses even with no GPU."""
    L = capi.lib()
    INVALID = -1
    ptr = C.c_void_p(4096)    # never dereferenced: every call below fails before a device is touched, or has nothing to do

    def knn(n=10, m=10, n_feat=3, n_seg=2, X=ptr, ldx=3, segptr=ptr, Q=ptr, ldq=3, qsegptr=ptr, k=4, flags=0, idx=ptr, ldi=4, dist=ptr,
            ldd=4):
        return L.gnnx_knn_f32(n, m, n_feat, n_seg, X, ldx, segptr, Q, ldq, qsegptr, k, flags, idx, ldi, dist, ldd, None)

    for name in ("n", "m"):
        assert knn(**{name: -1}) == INVALID, name
    assert knn(n_feat=0) == INVALID and knn(n_feat=-3) == INVALID
    assert knn(k=0) == INVALID and knn(k=kr.MAX_K + 1, ldi=100, ldd=100) == INVALID and knn(k=-1) == INVALID
    assert knn(ldx=2) == INVALID and knn(ldq=2) == INVALID
    assert knn(ldi=3) == INVALID and knn(ldd=3) == INVALID
    assert knn(flags=4) == INVALID and knn(flags=0x80000001) == INVALID
    assert knn(n_seg=0) == INVALID and knn(n_seg=-1) == INVALID
    assert knn(segptr=None) == INVALID and knn(qsegptr=None) == INVALID          # exactly one of the two while Q is given
    assert b"segment" in L.gnnx_last_error()
    assert knn(segptr=None, qsegptr=None, n_seg=2) == INVALID                     # both null: one segment only
    assert knn(Q=None, segptr=None, n_seg=2) == INVALID
    assert knn(Q=None, m=9) == INVALID                                            # the queries are the candidates: m == n
    assert knn(X=None) == INVALID and knn(idx=None) == INVALID
    assert b"null" in L.gnnx_last_error()
    # valid empty results need no device: no queries (idx may be null then; so may X without candidates)
    assert knn(m=0, idx=None, dist=None) == 0
    assert knn(m=0, n=0, X=None, idx=None) == 0
    assert knn(m=0, n=0, Q=None, X=None, idx=None, qsegptr=None) == 0
    assert knn(m=0, segptr=None, qsegptr=None, n_seg=1, dist=None, ldd=0) == 0   # ldd is read with d_dist only
    assert knn(m=0, Q=None, n=0, ldq=0, X=None) == 0                              # ldq with d_Q only
    assert knn(m=0, k=kr.MAX_K, ldi=kr.MAX_K, ldd=kr.MAX_K) == 0


def test_python_surface():
    ops = importlib.import_module("gnncpp_amd.ops")

    def params(f):
        return list(inspect.signature(f).parameters)

    assert params(ops.knn) == ["X", "k", "Q", "segptr", "qsegptr", "exclude_self", "nearest_first", "want_dist"]
    assert params(ops.knn_graph) == ["X", "k", "graph_ptr", "loop", "transpose", "norm"]
    assert params(ops.GraphBatch.of_points)[0] == "graph_ptr"
    assert params(ops.EdgeConvStack.__init__)[:5] == ["self", "g", "dims", "k", "seed"]
    assert issubclass(ops.EdgeConvStack, ops._Stack)
    for name in ("forward", "backward", "step", "train_step", "evaluate", "grad_buffer", "_bind", "on_graph"):
        assert callable(getattr(ops.EdgeConvStack, name)), name
    for name in ("step", "train_step", "evaluate", "grad_buffer"):                # the shared base's, not copies
        assert getattr(ops.EdgeConvStack, name) is getattr(ops.SageStack, name), name
    assert "Phi - Theta" in ops.EdgeConvStack.__doc__
    assert (ops.KNN_MAX_K, ops.KNN_EXCLUDE_SELF, ops.KNN_NEAREST_FIRST) == (kr.MAX_K, kr.EXCLUDE_SELF, kr.NEAREST_FIRST)
    with pytest.raises(ValueError):
        ops.EdgeConvStack(None, [3, 4], k=65)
