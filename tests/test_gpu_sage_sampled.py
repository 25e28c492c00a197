"""GPU tests of SageStack steps on sampled neighbourhoods (run with -m gpu on an MI355X): net.on_graph(g.sample_neighbors(k, seed)) on the
uniform graph with N = 1024 and E = 8000 (no row longer than 64), dims [16, 32, 16], every third row labelled, for both aggregators.

Bars: with k = 64 the sample IS the graph, so a step through the on_graph view must leave the loss and every parameter with the BITS of
a step of a stack on the full graph -- a wrong transposed CSR, inv_deg / map_t or buffer sharing shows here; with k = 5 the aggregated M
of layer 0 (for max also the arg) equals tests/spmm_ref.py / tests/reduce_ref.py on tests/sample_ref.py's CSR bit for bit; 30 epochs
with one seed each lower the FULL-graph loss; the run repeats bit for bit; the view holds the parent's parameter tensors."""
import importlib

import numpy as np
import pytest

from tests.helpers import synth
from tests.reduce_ref import spmm_reduce_ref
from tests.sample_ref import sample_ref
from tests.spmm_ref import spmm_ref

pytestmark = pytest.mark.gpu

N, E, DIMS = 1 << 10, 8000, [16, 32, 16]
LR = 0.05
AGGRS = ["mean", "max"]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    return dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def task(env):
    ops = env["ops"]
    src, dst = synth.uniform_edges(91, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    g.make_plans(64, max(DIMS))
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    deg = np.diff(rowptr)
    assert deg.max() <= 64 and deg.max() > 5
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32)
    rows = np.arange(0, N, 3, dtype=np.int32)
    return dict(g=g, rowptr=rowptr, colidx=colidx, deg=deg, X=X, target=target, rows=rows,
                dX=dev(env, X), dtarget=dev(env, target), drows=dev(env, rows))


def make_net(env, g, aggr, seed=950):
    net = env["ops"].SageStack(g, DIMS, aggr=aggr, seed=seed)
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    return net


def params(net):
    return net.W_s + net.W_n + net.b


@pytest.mark.parametrize("aggr", AGGRS)
def test_a_sample_that_is_the_graph_steps_with_the_full_graphs_bits(env, task, aggr):
    torch, g = env["torch"], task["g"]
    gs = g.sample_neighbors(64, seed=3)
    assert torch.equal(gs.rowptr, g.rowptr) and torch.equal(gs.colidx, g.colidx)
    assert torch.equal(gs.rowptr_t, g.rowptr_t) and torch.equal(gs.colidx_t, g.colidx_t)
    full, sampled = make_net(env, g, aggr), make_net(env, g, aggr)
    view = sampled.on_graph(gs)
    assert view.g is gs and sampled.g is g
    for step in range(3):
        a = full.train_step(task["dX"], task["dtarget"], task["drows"], lr=LR)
        b = view.train_step(task["dX"], task["dtarget"], task["drows"], lr=LR)
        assert torch.equal(a, b), f"loss of step {step}"
        for p, q in zip(params(full), params(sampled)):
            assert torch.equal(p, q), f"a parameter after step {step}"
    assert not torch.equal(full.W_n[0], make_net(env, g, aggr).W_n[0])        # the steps did move the parameters


@pytest.mark.parametrize("aggr", AGGRS)
def test_layer_zero_aggregates_the_reference_sample(env, task, aggr):
    k, seed = 5, 0
    net = make_net(env, task["g"], aggr)
    view = net.on_graph(task["g"].sample_neighbors(k, seed=seed))
    view.forward(task["dX"])
    _, M, arg, _ = view._saved[0]
    rp, ci, _, _ = sample_ref(task["rowptr"], task["colidx"], k, seed)
    assert (np.diff(rp) == np.minimum(task["deg"], k)).all() and rp[-1] < task["rowptr"][-1]
    if aggr == "mean":
        d = np.diff(rp)
        inv_deg = np.where(d > 0, np.float32(1) / np.maximum(d, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        assert np.array_equal(host(view.inv_deg), inv_deg)
        M_ref = spmm_ref(rp, ci, task["X"], rowscale=inv_deg)
    else:
        M_ref, arg_ref = spmm_reduce_ref(rp, ci, task["X"], None, "max")
        assert np.array_equal(host(arg), arg_ref)
    assert np.array_equal(host(M).view(np.int32), M_ref.view(np.int32))


@pytest.mark.parametrize("aggr", AGGRS)
def test_sampled_training_lowers_the_full_graph_loss_and_repeats(env, task, aggr):
    torch, g = env["torch"], task["g"]
    X, t, rows = task["dX"], task["dtarget"], task["drows"]
    runs = []
    for _ in range(2):
        net = make_net(env, g, aggr)
        before = float(host(net.evaluate(X, t, rows)[0])[0])
        losses = []
        for epoch in range(30):
            view = net.on_graph(g.sample_neighbors(5, seed=epoch))
            assert all(p is q for p, q in zip(params(view) + view.dW_s + view.dW_n + view.db, params(net) + net.dW_s + net.dW_n + net.db))
            assert view._buf is net._buf and view.g is not g and net.g is g
            losses.append(float(host(view.train_step(X, t, rows, lr=LR))[0]))
        after = float(host(net.evaluate(X, t, rows)[0])[0])
        assert all(np.isfinite(losses)) and np.isfinite(after)
        assert after < before, (before, after)
        runs.append((losses, after, [p.clone() for p in params(net)]))
    print(f"{aggr}: full-graph loss {before:.4f} -> {after:.4f}; sampled loss {runs[0][0][0]:.4f} -> {runs[0][0][-1]:.4f}")
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for p, q in zip(runs[0][2], runs[1][2]):
        assert torch.equal(p, q)


def test_on_graph_refuses_another_vertex_count(env, task):
    ops = env["ops"]
    src, dst = synth.uniform_edges(5, 64, 300)
    small = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), 64)
    with pytest.raises(ValueError):
        make_net(env, task["g"], "mean").on_graph(small)
