"""CPU-side checks of the bf16 dense segment attention calls: declared, exported, in the ctypes table; the f32 calls' status table comes
back before any HIP call (null device pointers, no GPU needed); a call that mixes bf16 and f32 operands is refused naming the tensor."""
import importlib

import pytest

from tests.helpers import pkg  # noqa: F401
from tests.test_cabi_cpu import capi  # noqa: F401 (the module fixture: builds and imports)

FWD, ROWS, COLS = "gnnx_segment_attn_bf16_f32", "gnnx_segment_attn_bwd_rows_bf16_f32", "gnnx_segment_attn_bwd_cols_bf16_f32"


def call(L, name, n_seg=2, n_rows=8, H=2, D=4, ld=8, ldo=8, beta=0.0):
    head = [n_seg, n_rows, None, H, D, 0.5]
    mats = [None, ld, None, ld, None, ld]   # Q, K, V
    if name == FWD:
        return getattr(L, name)(*head, *mats, None, ldo, None, None, None)
    if name == ROWS:
        return getattr(L, name)(*head, None, ld, *mats, None, ld, None, None, None, ldo, None, None)
    return getattr(L, name)(*head, None, ld, *mats, None, None, None, beta, None, ldo, None, ldo, None)


def test_symbols(capi):
    assert all(n in capi.declared_symbols() and n in capi._SIGS and hasattr(capi.lib(), n) for n in (FWD, ROWS, COLS))


@pytest.mark.parametrize("name", [FWD, ROWS, COLS])
@pytest.mark.parametrize("change,status", [(dict(n_rows=-1), -1), (dict(n_seg=-1), -1), (dict(H=0), -1), (dict(D=0), -1), (dict(ld=7), -1),
                                           (dict(ldo=7), -1), (dict(n_seg=0), -1), ({}, -1), (dict(D=129, ld=258, ldo=258), -7),
                                           (dict(n_rows=0), 0), (dict(n_seg=0, n_rows=0), 0)],
                         ids=["n_rows", "n_seg", "heads", "dim", "ld", "ld_out", "rows_without_segment", "null", "dim_129", "no_rows", "nothing"])
def test_statuses(capi, name, change, status):
    assert call(capi.lib(), name, **change) == status


def test_beta_and_mixed_operands(capi):
    import torch
    assert call(capi.lib(), COLS, beta=0.5) == -1
    ops = importlib.import_module("gnncpp_amd.ops")
    segptr = torch.tensor([0, 4], dtype=torch.int32)
    q, k = torch.zeros((4, 8), dtype=torch.bfloat16), torch.zeros((4, 8))
    with pytest.raises(capi.GnnxError, match="K must be torch.bfloat16"):   # host tensors: refused before any device call
        ops.segment_attention(segptr, q, k, q, 2)
    with pytest.raises(capi.GnnxError, match="Y must be torch.float32"):
        ops.segment_attention_bwd_rows(segptr, q, q, q, q, q, 2, k, k)
