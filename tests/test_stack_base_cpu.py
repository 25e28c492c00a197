"""CPU checks of what the stacks share (gnn.cpp_amd/ops.py, _Model / _Stack): import only, no device.  on_graph, the layer helpers and
the three statements that end an __init__ exist ONCE, in the base; every class keeps the parameter lists of __init__ and backward it
had before the shared copies were made."""
import importlib
import inspect

import pytest

STACKS = ["GcnStack", "GatStack", "Gatv2Stack", "SageStack", "EdgeConvStack", "GineStack", "TransformerStack", "RgcnStack", "PnaStack"]
MODEL_HELPERS = ["_init_state"]
STACK_HELPERS = ["on_graph", "_top_grad", "_bias_act", "_relu_tail", "_fused_tail"]
MODULE_HELPERS = ["_uniform_layers", "_zero_layers", "_need_transposed", "_edge_maps"]

BACKWARD = ["self", "dOut", "input_grad", "have_last_bias_grad"]
# the lists of the commit before the shared copies, written out
SIGNATURES = {
    "GcnStack": (["self", "g", "dims", "seed", "device", "pad_streamed"],
                 ["self", "dOut", "fused", "input_grad", "have_last_bias_grad", "labelled"]),
    "GatStack": (["self", "g", "dims", "negative_slope", "seed", "device", "heads", "fused"], BACKWARD),
    "Gatv2Stack": (["self", "g", "dims", "negative_slope", "seed", "device", "heads", "share_weights"], BACKWARD),
    "SageStack": (["self", "g", "dims", "aggr", "seed", "device"], BACKWARD),
    "EdgeConvStack": (["self", "g", "dims", "k", "seed", "device"], BACKWARD),
    "GineStack": (["self", "g", "dims", "edge_dim", "seed", "device"], BACKWARD),
    "TransformerStack": (["self", "g", "dims", "heads", "edge_dim", "global_attention", "seed", "device"], BACKWARD),
    "RgcnStack": (["self", "g", "dims", "n_relations", "n_bases", "norm", "seed", "device"], BACKWARD),
    "PnaStack": (["self", "g", "dims", "scalers", "eps", "seed", "device"], BACKWARD),
    "GraphClassifier": (["self", "net", "batch", "n_classes", "pool", "seed"], ["self", "dlogits", "have_bias_grad"]),
}


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("gnncpp_amd.ops")


def params(f):
    return list(inspect.signature(f).parameters)


def test_the_helpers_exist_once(ops):
    for name in MODEL_HELPERS:
        assert callable(ops._Model.__dict__[name]), name
    for name in STACK_HELPERS:
        assert callable(ops._Stack.__dict__[name]), name
    for name in MODULE_HELPERS:
        assert callable(getattr(ops, name)), name
    for cls in [getattr(ops, c) for c in STACKS] + [ops._AttentionStack, ops.GraphClassifier]:
        assert issubclass(cls, ops._Model)
        for name in MODEL_HELPERS + STACK_HELPERS:
            assert name not in cls.__dict__, (cls.__name__, name)


@pytest.mark.parametrize("name", STACKS)
def test_on_graph_is_the_base_method(ops, name):
    cls = getattr(ops, name)
    assert issubclass(cls, ops._Stack)
    assert cls.on_graph is ops._Stack.on_graph
    assert params(cls.on_graph) == ["self", "g"]


def test_on_graph_documents_sharing_and_the_gather_pitch(ops):
    doc = " ".join(ops._Stack.on_graph.__doc__.split())
    for phrase in ("SHARES", "zeroed-rows mark", "net.on_graph(g.sample_neighbors(k, seed=epoch)).train_step(X, target, rows, lr)", "gather pitch"):
        assert phrase in doc, phrase
    assert "SageStack.on_graph" not in inspect.getsource(ops)
    assert "any stack" in ops.GraphClassifier.__doc__ and "three stacks" not in ops.GraphClassifier.__doc__


@pytest.mark.parametrize("name", STACKS + ["GraphClassifier"])
def test_no_class_keeps_a_pasted_copy(ops, name):
    src = inspect.getsource(getattr(ops, name))
    assert "self._opt = [None]" not in src and "_view(share_buf=True)" not in src
    assert "self._init_state()" in src


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_are_the_parents(ops, name):
    cls = getattr(ops, name)
    init, backward = SIGNATURES[name]
    assert params(cls.__init__) == init
    assert params(cls.backward) == backward


def test_arguments_are_checked_before_the_graph_is_touched(ops):
    with pytest.raises(ValueError):
        ops.EdgeConvStack(None, [3, 4], k=65)
    with pytest.raises(ValueError):
        ops.SageStack(None, [3, 4], aggr="sum")
    with pytest.raises(ValueError):
        ops.RgcnStack(None, [3, 4], 2, norm="max")
    with pytest.raises(ValueError):
        ops.PnaStack(None, [3, 4], scalers=("identity", "identity"))


def test_graph_requirements_keep_their_errors(ops):
    capi = importlib.import_module("gnncpp_amd.capi")

    class G:
        rowptr_t = colidx_t = None

    with pytest.raises(capi.GnnxError, match=r"the graph has no transposed CSR \(from_coo\(\.\.\., transpose=True\)\)") as e:
        ops._need_transposed(G(), "SageStack")
    assert "SageStack" in str(e.value)
    with pytest.raises(capi.GnnxError, match=r"the graph has no edge attributes \(g\.set_edge_attr\(src, dst, attr\)\)") as e:
        ops._edge_maps(G(), 3, "GineStack")
    assert "GineStack" in str(e.value)

    class Attributed(G):
        class edge_attr:
            shape = (7, 2)
        entry_edge, entry_edge_t = "map", "map_t"

    with pytest.raises(ValueError, match="the graph's edge attributes have 2 columns, the stack was built for 3"):
        ops._edge_maps(Attributed(), 3, "TransformerStack")
    assert ops._edge_maps(Attributed(), 2, "TransformerStack") == ("map", "map_t")
