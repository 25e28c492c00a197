"""CPU-side checks of the cross segment attention calls: declared, exported, in the ctypes table; every status the header lists comes back
before any HIP call (null device pointers, no GPU needed); the classifier refuses a readout its stack's width cannot serve."""
import importlib

import pytest

from tests.helpers import pkg  # noqa: F401
from tests.test_cabi_cpu import capi  # noqa: F401 (the module fixture: builds and imports)

FWD, ROWS, COLS = "gnnx_segment_cross_attn_f32", "gnnx_segment_cross_attn_bwd_rows_f32", "gnnx_segment_cross_attn_bwd_cols_f32"


def call(L, name, n_seg=2, n_rows=8, n_q=4, H=2, D=4, ld=8, ldo=8, beta=0.0):
    head = [n_seg, n_rows, None, n_q, None, H, D, 0.5]
    mats = [None, ld, None, ld, None, ld]   # Q, K, V
    if name == FWD:
        return getattr(L, name)(*head, *mats, None, ldo, None, None, None)
    if name == ROWS:
        return getattr(L, name)(*head, None, ld, *mats, None, ld, None, None, None, ldo, None, None)
    return getattr(L, name)(*head, None, ld, *mats, None, None, None, beta, None, ldo, None, ldo, None)


def test_symbols(capi):
    assert all(n in capi.declared_symbols() and n in capi._SIGS and hasattr(capi.lib(), n) for n in (FWD, ROWS, COLS))


@pytest.mark.parametrize("name", [FWD, ROWS, COLS])
@pytest.mark.parametrize("change,status", [(dict(n_rows=-1), -1), (dict(n_seg=-1), -1), (dict(n_q=-1), -1), (dict(H=0), -1), (dict(D=0), -1),
                                           (dict(ld=7), -1), (dict(ldo=7), -1), (dict(n_seg=0), -1), ({}, -1), (dict(D=129, ld=258, ldo=258), -7),
                                           (dict(n_q=0, n_rows=0), 0), (dict(n_seg=0, n_rows=0, n_q=0), 0)],
                         ids=["n_rows", "n_seg", "n_q", "heads", "dim", "ld", "ld_out", "rows_without_segment", "null", "dim_129", "no_rows", "nothing"])
def test_statuses(capi, name, change, status):
    assert call(capi.lib(), name, **change) == status


def test_empty_sides_beta_and_the_readout_option(capi):
    L = capi.lib()
    assert call(L, FWD, n_q=0) == 0 and call(L, ROWS, n_q=0) == 0     # no query: a valid empty result
    assert call(L, COLS, n_q=0) == -1 and call(L, COLS, n_rows=0) == 0   # no query still writes beta * old: null outputs are refused
    assert call(L, COLS, beta=0.5) == -1
    ops = importlib.import_module("gnncpp_amd.ops")
    net = object.__new__(ops.GcnStack)
    net.dims = [4, 8]   # the width is checked before the graph is touched
    with pytest.raises(ValueError, match="heads"):
        ops.GraphClassifier(net, None, 3, pool=ops.AttentionReadout(heads=3))
    with pytest.raises(ValueError, match="pool"):
        ops.GraphClassifier(net, None, 3, pool="attention")
