"""CPU-side checks of semi-supervised (masked) training: the new C-ABI entry points are declared, exported and bound; the C++
mirror offers Data::set_mask / DataType / the masked loss and accuracy; set_mask refuses a wrong-sized mask with the reference's
message (src/graph.cpp:130-151).  The numerics are tests/test_gpu_masked.py."""
import ctypes as C
import importlib
import inspect
import os
import subprocess

import pytest

from tests.helpers import ROOT, pkg  # noqa: F401

NEW_SYMBOLS = ["gnnx_mask_to_rows_workspace", "gnnx_mask_to_rows", "gnnx_csr_restrict_workspace", "gnnx_csr_restrict",
               "gnnx_softmax_ce_rows_workspace", "gnnx_softmax_ce_rows_f32", "gnnx_argmax_rows_workspace", "gnnx_argmax_rows_f32",
               "gnnx_accuracy_rows_f32"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_masked_entry_points_are_declared_exported_and_bound(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in declared, f"include/gnnx.h does not declare {n}"
        assert hasattr(L, n), f"libgnnx_hip.so does not export {n}"
        assert n in capi._SIGS, f"capi.py has no signature for {n}"
    header = open(capi.HEADER_PATH).read()
    block = header[header.index("semi-supervised training: masks"):header.index("gnnx_mask_to_rows_workspace(")]
    assert "graph.cpp:130-151" in block and "functional.h:59-61" in block and "nn.cpp:442-453" in block


def test_masked_argument_validation_without_device(capi):
    """What the entry points refuse before they touch a device."""
    L = capi.lib()
    b = C.c_size_t(0)
    assert L.gnnx_softmax_ce_rows_workspace(10, 7, C.byref(b)) == 0 and b.value > 0
    assert L.gnnx_argmax_rows_workspace(C.byref(b)) == 0 and b.value > 0
    assert L.gnnx_softmax_ce_rows_workspace(-1, 7, C.byref(b)) == -1
    # an empty row list is an error, never a NaN loss
    assert L.gnnx_softmax_ce_rows_f32(None, 7, None, None, 0, 10, 7, 0, None, None, 0, None, None, 0, None) == -1
    assert "empty row list" in L.gnnx_last_error().decode()
    cnt = C.c_int32(5)
    assert L.gnnx_mask_to_rows(None, 0, None, C.byref(cnt), None, 0, None) == 0 and cnt.value == 0
    assert L.gnnx_mask_to_rows(None, -1, None, C.byref(cnt), None, 0, None) == -1
    nnz = C.c_int64(0)
    assert L.gnnx_csr_restrict(-1, 0, 0, None, None, None, None, None, None, None, None, C.byref(nnz), None, 0, None) == -1
    correct = C.c_int64(9)
    assert L.gnnx_accuracy_rows_f32(None, 7, None, None, 0, 0, 7, None, C.byref(correct), None, 0, None) == 0 and correct.value == 0


def test_python_layer_offers_the_masked_training_api(capi):
    ops = importlib.import_module("gnncpp_amd.ops")
    for name in ("rows_from_mask", "csr_restrict", "softmax_ce_rows", "argmax_rows", "accuracy"):
        assert callable(getattr(ops, name))
    assert list(inspect.signature(ops.softmax_ce_rows).parameters) == ["logits", "target", "rows", "colsum_out", "grad_out", "n_total",
                                                                        "want_grad"]
    for fn in (ops.aggregate_fwd, ops.aggregate_bwd, ops.GcnStack.forward, ops.GcnStack.backward):
        assert inspect.signature(fn).parameters["labelled"].default is None   # every new argument defaults to today's behaviour
    for name in ("labelled", "rows_of"):
        assert callable(getattr(ops.CsrGraph, name))
    for name in ("train_step", "evaluate"):
        assert callable(getattr(ops.GcnStack, name))


SNIPPET = r"""
#include "graph.h"
#include "nn.h"
#include "tensor.h"
float use(graph::Data &data, cyg::tptr<float> logits, cyg::tptr<int> target, cyg::tensor<bool> &train, cyg::tensor<bool> &val)
{
    data.set_mask(train);                                   // DataType::TRAIN by default, as in the reference
    data.set_mask(val, graph::DataType::VAL);
    data.set_mask(val, graph::DataType::TEST);
    graph::DataType t = graph::DataType::TRAIN;
    (void)t;
    cyg::tensor<bool> *m = data.train_mask();
    cyg::tptr<float> loss = nn::cross_entropy_loss(logits, target, *m);
    loss->backward();
    size_t hits = nn::count_correct(logits, target, *data.val_mask());
    return nn::accuracy(logits, target, *data.test_mask()) + (float)hits;
}
"""


def test_mirror_call_sites_compile(tmp_path):
    src = tmp_path / "masked_call_sites.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wno-sign-compare", "-I" + os.path.join(ROOT, "gnn.cpp_amd", "host", "include"),
                        "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_set_mask_conventions_cpu(capi):
    """tests/cpp/test_host_masked_cpu.cpp: masks are stored per DataType; a wrong-sized mask throws the reference's message."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_host_masked_cpu")
    assert os.path.exists(exe), "build() did not produce tests/cpp/test_host_masked_cpu"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "masked host api (cpu) ok" in r.stdout, r.stdout + r.stderr
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_host_masked_gpu"))
