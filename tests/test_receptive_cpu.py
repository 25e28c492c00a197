"""CPU-side checks of query inference (receptive fields): the new C-ABI entry points are declared, exported and bound, their header
block cites the reference lines the feature stands on, the argument checks that need no device return the stated codes, the Python
layer offers the API, and the numpy yardstick of tests/test_gpu_receptive.py (tests/receptive_ref.py) gives hand-written
expectations on the reference's 8-edge graph and on a path graph.  The numerics are tests/test_gpu_receptive.py."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest

import oracle
from tests.golden_util import load_case
from tests.helpers import ROOT, pkg  # noqa: F401
from tests.receptive_ref import ref_extract, ref_field, ref_frontier

NEW_SYMBOLS = ["gnnx_frontier_mark_workspace", "gnnx_frontier_mark", "gnnx_rows_to_positions_workspace", "gnnx_rows_to_positions",
               "gnnx_csr_extract_rows_workspace", "gnnx_csr_extract_rows"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_receptive_entry_points_are_declared_exported_and_bound(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in declared, f"include/gnnx.h does not declare {n}"
        assert hasattr(L, n), f"libgnnx_hip.so does not export {n}"
        assert n in capi._SIGS, f"capi.py has no signature for {n}"
    header = open(capi.HEADER_PATH).read()
    block = header[header.index("query inference: receptive fields"):header.index("gnnx_frontier_mark_workspace(")]
    assert "graph.cpp:170-191" in block and "graph.cpp:68-75" in block and "graph.cpp:130-151" in block


def test_receptive_argument_validation_without_device(capi):
    """What the entry points decide before they touch a device."""
    L = capi.lib()
    INVALID = -1
    b = C.c_size_t(0)
    assert L.gnnx_rows_to_positions_workspace(C.byref(b)) == 0 and b.value > 0
    assert L.gnnx_frontier_mark_workspace(-1, C.byref(b)) == INVALID
    assert L.gnnx_csr_extract_rows_workspace(-1, C.byref(b)) == INVALID
    nnz = C.c_int64(7)
    # negative sizes, each with a message
    for args in ((-1, 5, 0), (5, -1, 0), (5, 5, -1)):
        n_rows, n_cols, n_listed = args
        assert L.gnnx_frontier_mark(None, None, n_rows, n_cols, None, n_listed, None, C.byref(nnz), None, 0, None) == INVALID
        assert "negative size" in L.gnnx_last_error().decode()
    assert L.gnnx_rows_to_positions(None, -1, 5, None, None, 0, None) == INVALID
    assert L.gnnx_rows_to_positions(None, 0, -1, None, None, 0, None) == INVALID
    assert "negative size" in L.gnnx_last_error().decode()
    for n_rows, n_cols, n_listed, cap in ((-1, 5, 0, 0), (5, -1, 0, 0), (5, 5, -1, 0), (5, 5, 0, -1)):
        assert L.gnnx_csr_extract_rows(n_rows, n_cols, None, None, None, None, n_listed, None, None, None, None, cap, C.byref(nnz), None, 0,
                                       None) == INVALID
        assert "negative size" in L.gnnx_last_error().decode()
    # no listed rows: nothing to mark, no entries -- a result, not an error
    nnz.value = 7
    assert L.gnnx_frontier_mark(None, None, 5, 5, None, 0, None, C.byref(nnz), None, 0, None) == 0 and nnz.value == 0
    assert L.gnnx_rows_to_positions(None, 0, 0, None, None, 0, None) == 0
    # more listed rows than rows cannot be ascending without repeats
    assert L.gnnx_frontier_mark(None, None, 5, 5, None, 6, None, C.byref(nnz), None, 0, None) == INVALID
    assert L.gnnx_csr_extract_rows(5, 5, None, None, None, None, 6, None, None, None, None, 0, C.byref(nnz), None, 0, None) == INVALID
    assert L.gnnx_rows_to_positions(None, 6, 5, None, None, 0, None) == INVALID
    # the count pointer is required
    assert L.gnnx_frontier_mark(None, None, 5, 5, None, 0, None, None, None, 0, None) == INVALID


def test_python_layer_offers_the_query_inference_api(capi):
    ops = importlib.import_module("gnncpp_amd.ops")
    for name in ("frontier", "csr_extract_rows", "rows_to_positions"):
        assert callable(getattr(ops, name))
    assert list(inspect.signature(ops.frontier).parameters) == ["rowptr", "colidx", "rows", "n_cols"]
    assert list(inspect.signature(ops.CsrGraph.receptive_field).parameters) == ["self", "query", "n_layers"]
    assert list(inspect.signature(ops.GcnStack.predict).parameters) == ["self", "X", "field"]
    assert list(inspect.signature(ops.GcnStack.evaluate_field).parameters) == ["self", "X", "target", "field"]
    assert inspect.isclass(ops.ReceptiveField)
    # evaluate itself is unchanged
    assert list(inspect.signature(ops.GcnStack.evaluate).parameters) == ["self", "X", "target", "rows"]


# ------------------------------------------------------------------ the yardstick of the GPU tests, by hand
def test_ref_field_on_the_reference_test_graph():
    """tests/graph.test.cpp:19-20 of the reference (golden fixture testgraph_n5): 8 edges, 2 of them self loops, which the adjacency
    drops (graph.cpp:68-75).  Rows: 0 -> {1}, 1 -> {2}, 2 -> {1}, 3 -> {0, 1}, 4 -> {2}."""
    case = load_case("testgraph_n5")
    rowptr, colidx = oracle.coo_to_csr(case["src"], case["dst"], 5)
    assert rowptr.tolist() == [0, 1, 2, 3, 5, 6] and colidx.tolist() == [1, 2, 1, 0, 1, 2]
    cols, n_ent = ref_frontier(rowptr, colidx, [3])
    assert cols.tolist() == [0, 1] and n_ent == 2 and cols.dtype == np.int32
    f = ref_field(rowptr, colidx, [3], 2)
    assert [r.tolist() for r in f["rows"]] == [[1, 2], [0, 1], [3]]
    assert f["nnz"] == [0, 2, 2]
    assert f["blocks"][2][0].tolist() == [0, 2] and f["blocks"][2][1].tolist() == [0, 1]
    assert f["blocks"][1][0].tolist() == [0, 1, 2] and f["blocks"][1][1].tolist() == [0, 1]
    assert f["query_pos"].tolist() == [0]
    # an unsorted query with a repeat: Q_1 is the unique ascending set, every query entry knows its compact row
    f = ref_field(rowptr, colidx, [4, 0, 4], 1)
    assert [r.tolist() for r in f["rows"]] == [[1, 2], [0, 4]]
    assert f["blocks"][1][0].tolist() == [0, 1, 2] and f["blocks"][1][1].tolist() == [0, 1]
    assert f["query_pos"].tolist() == [1, 0, 1]
    # vertex 1's two-hop field is {1, 2}: 1 -> {2} -> {1}; a vertex is in its own field only through a neighbour
    f = ref_field(rowptr, colidx, [1], 2)
    assert [r.tolist() for r in f["rows"]] == [[1], [2], [1]]
    # every vertex: layer 1 reads columns {0, 1, 2} only (nobody points at 3 or 4)
    f = ref_field(rowptr, colidx, np.arange(5), 1)
    assert f["rows"][0].tolist() == [0, 1, 2] and f["nnz"][1] == 6
    assert f["blocks"][1][0].tolist() == rowptr.tolist() and f["blocks"][1][1].tolist() == colidx.tolist()


def test_ref_field_on_a_path_graph():
    """0 - 1 - 2 - 3 - 4 - 5, both directions: the field of an end vertex grows by one vertex per hop and alternates parity."""
    n = 6
    rowptr = np.array([0, 1, 3, 5, 7, 9, 10])
    colidx = np.array([1, 0, 2, 1, 3, 2, 4, 3, 5, 4])
    f = ref_field(rowptr, colidx, [0], 3)
    assert [r.tolist() for r in f["rows"]] == [[1, 3], [0, 2], [1], [0]]
    assert f["nnz"] == [0, 3, 2, 1]
    assert f["blocks"][3][0].tolist() == [0, 1] and f["blocks"][3][1].tolist() == [0]
    assert f["blocks"][2][0].tolist() == [0, 2] and f["blocks"][2][1].tolist() == [0, 1]
    assert f["blocks"][1][0].tolist() == [0, 1, 3] and f["blocks"][1][1].tolist() == [0, 0, 1]
    f = ref_field(rowptr, colidx, np.arange(n), 2)
    assert all(r.tolist() == list(range(n)) for r in f["rows"])


def test_ref_extract_keeps_stored_order_and_refuses_a_missing_column():
    """Row 0 stores its columns as 2, 1 (a relabelled graph's rows are sorted by ORIGINAL column id); row 1 is isolated."""
    rowptr, colidx = np.array([0, 2, 2, 3]), np.array([2, 1, 0])
    vals = np.array([0.5, 0.25, 4.0], dtype=np.float32)
    rp, ci, v = ref_extract(rowptr, colidx, [0], col_set=[1, 2], vals=vals)
    assert rp.tolist() == [0, 2] and ci.tolist() == [1, 0] and v.tolist() == [0.5, 0.25]
    rp, ci, v = ref_extract(rowptr, colidx, [0, 2], vals=vals)           # no set: the column ids themselves
    assert rp.tolist() == [0, 2, 3] and ci.tolist() == [2, 1, 0] and v.tolist() == [0.5, 0.25, 4.0]
    f = ref_field(rowptr, colidx, [1], 2)                                # an isolated vertex: empty frontier, a block of no entries
    assert [r.tolist() for r in f["rows"]] == [[], [], [1]] and f["nnz"] == [0, 0, 0]
    assert f["blocks"][2][0].tolist() == [0, 0] and f["blocks"][2][1].tolist() == []
    assert f["blocks"][1][0].tolist() == [0]
    rp, ci, _ = ref_extract(rowptr, colidx, [])                          # no rows: rowptr' = [0]
    assert rp.tolist() == [0] and ci.size == 0
    with pytest.raises(KeyError):
        ref_extract(rowptr, colidx, [0], col_set=[2])
    with pytest.raises(KeyError):
        ref_extract(rowptr, colidx, [0], col_set=[])
