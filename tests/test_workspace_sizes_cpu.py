"""Every `gnnx_*_workspace` query of include/gnnx.h that takes sizes only, held to recorded byte counts (tests/golden/workspace_sizes.json).

A query and its entry point carve the caller's workspace with the same code (gnnx_common.h `Carver`, gnnx_worklist.h `HubList`), so the
counts a query returns are the layout.  The fixture was recorded from the library as it stood BEFORE the carving was shared
(`python -m tests.test_workspace_sizes_cpu <libgnnx_hip.so> > tests/golden/workspace_sizes.json`); a change of any count is a change of
the C-ABI's contract and has to be made on purpose, with the fixture.  The shapes cross every threshold of the list capacities: rows
longer than 16 (edge softmax), 256 (sampler) and S = 4096 entries, nnz / S, nnz at the int32 limit, and feature counts 1, 4, 5, 64.
The queries whose count includes rocPRIM's own scratch (a figure of the rocPRIM release and the device, not of this project) return
GNNX_ERR_HIP without a device and stay out of the table, so that it does not depend on the machine: see `NEEDS_DEVICE`.  Their
layouts are held by the GPU suites of the graph build, the mask calls and the receptive field."""
import ctypes as C
import itertools
import json
import os
import re
import sys

import pytest

from tests.helpers import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
ROWS = (0, 1, 1000, 10 ** 7)
NNZ = (0, 16, 17, 256, 257, 4096, 4097, 5000, 10 ** 8, 2 ** 31 - 1)
FEAT = (1, 4, 5, 64)
ROLE = {"n_rows": ROWS, "n_nodes": ROWS, "n_seg": ROWS, "n_listed": ROWS, "M": ROWS,
        "nnz": NNZ, "n_edges": NNZ, "n": NNZ,
        "n_feat": FEAT, "n_classes": FEAT, "n_heads": FEAT, "k": FEAT, "N": FEAT, "K": FEAT,
        "transA": (0, 1), "transB": (0, 1)}
CTYPE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
# their count adds what rocprim::exclusive_scan / radix_sort ask for, which rocPRIM answers per device
NEEDS_DEVICE = {"gnnx_csr_from_coo_workspace", "gnnx_csr_from_coo_weighted_workspace", "gnnx_mask_to_rows_workspace",
                "gnnx_csr_restrict_workspace", "gnnx_frontier_mark_workspace", "gnnx_csr_extract_rows_workspace"}


def queries():
    """(name, ((type, parameter), ...)) of every workspace query whose parameters are integers and the `size_t *bytes` result."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnnx.h")).read(), flags=re.S)
    out = []
    for name, params in re.findall(r"\bint\s+(gnnx_[a-z0-9_]+_workspace)\s*\(([^)]*)\)\s*;", text):
        params = [p.split() for p in params.split(",")]
        if params[-1] != ["size_t", "*bytes"] or any(len(p) != 2 or p[0] not in CTYPE for p in params[:-1]):
            continue   # takes a plan or a pointer: not a function of sizes alone
        out.append((name, tuple((t, n) for t, n in params[:-1])))
    return out


def measure(L):
    """{query: [[arguments..., status, bytes], ...]} over the cross product of the shapes; bytes is 0 where the status is not."""
    table = {}
    for name, params in queries():
        if name in NEEDS_DEVICE:
            continue
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = [CTYPE[t] for t, _ in params] + [C.POINTER(C.c_size_t)]
        rows = []
        for args in itertools.product(*(ROLE[n] for _, n in params)):
            b = C.c_size_t(0)
            status = fn(*args, C.byref(b))
            rows.append(list(args) + [status, b.value if status == 0 else 0])
        table[name] = rows
    return table


def test_every_sizes_only_query_is_in_the_table():
    names = [n for n, _ in queries()]
    assert len(names) == len(set(names)) and len(names) >= 26
    for hub_unit in ("gnnx_edge_softmax_workspace", "gnnx_edge_softmax_heads_workspace", "gnnx_spmm_csr_reduce_workspace",
                     "gnnx_csr_sample_workspace", "gnnx_segment_pool_workspace", "gnnx_softmax_ce_rows_workspace"):
        assert hub_unit in names and hub_unit not in NEEDS_DEVICE
    assert NEEDS_DEVICE <= set(names)
    assert all(n in ROLE for _, params in queries() for _, n in params)


def test_workspace_sizes_are_the_recorded_ones():
    import importlib

    import __graft_entry__ as ge
    ge.build()
    got = measure(importlib.import_module("gnncpp_amd.capi").lib())
    want = json.load(open(FIXTURE))
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
    # the table is not vacuous: a first possible hub (S + 1 entries) and a first full segment (S entries) each move the count
    by_args = {tuple(r[:-2]): r[-1] for r in want["gnnx_spmm_csr_reduce_workspace"]}
    assert by_args[(1000, 4097, 64)] > by_args[(1000, 4096, 64)] > by_args[(1000, 257, 64)] == by_args[(1000, 0, 64)]


if __name__ == "__main__":
    json.dump(measure(C.CDLL(sys.argv[1])), sys.stdout, separators=(",", ":"))
