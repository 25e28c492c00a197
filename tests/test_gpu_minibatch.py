"""GPU tests of mini-batch GraphSAGE (run with -m gpu on an MI355X): CsrGraph.sampled_field / ops.SampledField and SageStack.predict /
batch_step on the uniform graph of tests/test_gpu_sage_sampled.py (N = 1024, E = 8000, no row longer than 64), dims [16, 32, 16], both
aggregators.

Bars.  Integers: every array of the field equals tests/minibatch_ref.py's.  Bits: with per-layer seeds [s, s] and fanouts [k, k] the
field is the 2-hop field of g.sample_neighbors(k, s) and every product is row-local, so predict must be torch.equal to that sampled
graph's forward at the seeds.  Float64: one batch_step against tests/minibatch_ref.py on the device's own field is held to the bars of
tests/test_gpu_sage.py::test_one_step_vs_float64, unchanged -- 1e-5 * max(1, |ref|) for the loss and 2e-5 * max(|ref|_max, 1e-3) for
every parameter gradient; for max the float64 model routes through the device's arg, whose choice must be a float64 maximiser to
1e-5, as there."""
import importlib

import numpy as np
import pytest

from tests import minibatch_ref as mr
from tests.helpers import synth

pytestmark = pytest.mark.gpu

N, E, DIMS = 1 << 10, 8000, [16, 32, 16]
LR = 0.05
AGGRS = ["mean", "max"]
SEEDS8 = np.array([700, 3, 512, 1023, 3, 64, 0, 999])          # unsorted, one repeated


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
    bare = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)        # the same graph without plans
    rowptr, colidx = host(g.rowptr), host(g.colidx)
    deg = np.diff(rowptr)
    assert deg.max() <= 64 and deg.max() > 5
    X = synth.uniform_pm1(93, (N, DIMS[0]))
    target = ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32)
    return dict(g=g, bare=bare, src=src, dst=dst, rowptr=rowptr, colidx=colidx, deg=deg, X=X, target=target, dX=dev(env, X),
                dtarget=dev(env, target), all_rows=dev(env, np.arange(N, dtype=np.int32)))


def make_net(env, g, aggr, seed=950):
    net = env["ops"].SageStack(g, DIMS, aggr=aggr, seed=seed)
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    return net


def params(net):
    return net.W_s + net.W_n + net.b


def assert_field_is_reference(field, ref, L):
    for l in range(L + 1):
        assert np.array_equal(host(field.rows[l]), ref["rows"][l]), f"rows[{l}]"
        assert host(field.rows[l]).dtype == np.int32
    assert np.array_equal(host(field.query_pos), ref["query_pos"])
    for l in range(1, L + 1):
        assert field.nnz[l] == ref["nnz"][l]
        for name, got, want in (("rowptr", field.block[l][0], ref["block"][l][0]), ("colidx", field.block[l][1], ref["block"][l][1]),
                                ("self_pos", field.self_pos[l], ref["self_pos"][l]), ("rowptr_t", field.block_t[l][0], ref["block_t"][l][0]),
                                ("colidx_t", field.block_t[l][1], ref["block_t"][l][1])):
            assert np.array_equal(host(got), want), f"{name} of layer {l}"
        assert np.array_equal(host(field.inv_deg[l]).view(np.int32), ref["inv_deg"][l].view(np.int32)), f"inv_deg of layer {l}"


def test_the_field_is_the_reference_field(env, task):
    g = task["g"]
    field = g.sampled_field(dev(env, SEEDS8), [5, 5], seed=7)
    ref = mr.field_ref(task["rowptr"], task["colidx"], SEEDS8, [5, 5], 7)
    assert field.seeds == [14, 15] == ref["seeds"] and field.n_query == 8 and field.n_layers == 2
    assert np.array_equal(host(field.query_rows), SEEDS8.astype(np.int32))
    assert_field_is_reference(field, ref, 2)
    sizes = [int(r.numel()) for r in field.rows]
    assert sizes[2] == 7 and sizes[1] <= 8 + 40 and sizes[0] <= 8 + 40 + 240 < N and sizes[0] > sizes[1] > sizes[2]
    ref2 = mr.field_ref(task["rowptr"], task["colidx"], SEEDS8, [3, 6], [21, 4])             # per-layer seeds, unequal fanouts
    assert_field_is_reference(g.sampled_field(dev(env, SEEDS8), [3, 6], seed=[21, 4]), ref2, 2)
    for bad in (dev(env, np.array([0, N])), dev(env, np.array([-1])), dev(env, np.zeros((2, 2), dtype=np.int64)), dev(env, np.zeros(3, dtype=np.float32))):
        with pytest.raises(ValueError):
            g.sampled_field(bad, [5, 5], seed=0)
    with pytest.raises(ValueError):
        g.sampled_field(dev(env, SEEDS8), [5, 5], seed=[1, 2, 3])


@pytest.mark.parametrize("planned", [True, False])
@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("aggr", AGGRS)
def test_predict_has_the_bits_of_the_sampled_graphs_forward(env, task, aggr, k, planned):
    torch = env["torch"]
    g, s = (task["g"] if planned else task["bare"]), 12
    assert (g.plan is not None) == planned
    net = make_net(env, g, aggr)
    seeds = np.concatenate([SEEDS8, np.arange(100, 164)])
    field = g.sampled_field(dev(env, seeds), [k, k], seed=[s, s])
    full = net.on_graph(g.sample_neighbors(k, s)).forward(task["dX"])
    step_logits = full.clone()
    got = net.predict(task["dX"], field)
    assert got.shape == (len(seeds), DIMS[-1])
    assert torch.equal(got, full[dev(env, seeds)])
    assert torch.equal(full, step_logits)                      # predict has buffers of its own: the forward's result stands
    if k == 64:                                                # the sample is the graph: the full forward itself
        assert torch.equal(got, net.forward(task["dX"])[dev(env, seeds)])


@pytest.mark.parametrize("aggr", AGGRS)
def test_isolated_single_and_whole_graph_batches(env, task, aggr):
    torch, ops = env["torch"], env["ops"]
    n_iso = N + 1                                              # vertex N has no edge at all
    g = ops.CsrGraph.from_coo(dev(env, task["src"]), dev(env, task["dst"]), n_iso)
    assert int(g.rowptr[N + 1] - g.rowptr[N]) == 0
    X = torch.cat([task["dX"], dev(env, synth.uniform_pm1(5, (1, DIMS[0])))])
    net = make_net(env, g, aggr)
    field = g.sampled_field(dev(env, np.array([N, 17])), [5, 5], seed=1)
    got = net.predict(X, field)
    h = X[N:]                                                  # the isolated vertex: W_s and b alone, layer after layer
    for l in range(2):
        h = ops.bias_add(ops.gemm(h.contiguous(), net.W_s[l], transB=True), net.b[l])
        h = h.clamp(min=0) if l == 0 else h
    assert torch.equal(got[0:1], h)
    alone = g.sampled_field(dev(env, np.array([N])), [5, 5], seed=1)    # one vertex as the whole batch, with no entry anywhere
    assert alone.nnz == [0, 0, 0] and [int(r.numel()) for r in alone.rows] == [1, 1, 1]
    assert torch.equal(net.predict(X, alone), h)
    loss = net.batch_step(X, torch.zeros(n_iso, dtype=torch.int32, device=env["dev"]), alone, lr=0.0)
    assert np.isfinite(host(loss)[0]) and bool((net.dW_n[0] == 0).all()) and bool((net.dW_n[1] == 0).all())
    one = task["g"].sampled_field(dev(env, np.array([5])), [5, 5], seed=[2, 2])  # one vertex with neighbours as the whole batch
    net1 = make_net(env, task["g"], aggr)
    assert task["deg"][5] > 0 and int(one.rows[2].numel()) == 1 and one.nnz[2] == min(5, task["deg"][5])
    ref = net1.on_graph(task["g"].sample_neighbors(5, 2)).forward(task["dX"])
    assert torch.equal(net1.predict(task["dX"], one), ref[5:6])
    everything = task["g"].sampled_field(task["all_rows"], [64, 64], seed=0)    # every vertex, k = 64: the field is the graph
    for l in (1, 2):
        assert torch.equal(everything.block[l][0], task["g"].rowptr) and torch.equal(everything.block[l][1], task["g"].colidx)
        assert torch.equal(everything.block_t[l][0], task["g"].rowptr_t) and torch.equal(everything.block_t[l][1], task["g"].colidx_t)
        assert torch.equal(everything.self_pos[l], task["all_rows"])
    assert torch.equal(net1.predict(task["dX"], everything), net1.forward(task["dX"]))


@pytest.mark.parametrize("aggr", AGGRS)
def test_one_batch_step_vs_float64(env, task, aggr):
    torch = env["torch"]
    g = task["g"]
    net = make_net(env, g, aggr)
    names = ("W_s", "W_n", "b")
    before = [p.clone() for k in names for p in getattr(net, k)]
    p64 = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in names}
    seeds = np.concatenate([SEEDS8, np.arange(300, 340)])
    field = g.sampled_field(dev(env, seeds), [5, 5], seed=3)
    saved = net._field_forward(task["dX"], field)
    args = [None if s[3] is None else host(s[3]) for s in saved]
    loss = net.batch_step(task["dX"], task["dtarget"], field, lr=0.0)
    f = dict(rows=[host(r) for r in field.rows], block=[None] + [(host(a), host(b)) for a, b in field.block[1:]],
             self_pos=[None] + [host(s) for s in field.self_pos[1:]])       # the device's own field
    logits, chosen = mr.forward64(torch, f, task["X"], p64, aggr, args)
    ref = mr.loss64(torch, logits, task["target"][f["rows"][2]])
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"{aggr}: loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for l, (true, picked) in enumerate(chosen):          # the device's winner is a float64 maximiser
        gap = np.abs(true - picked) / np.maximum(1.0, np.abs(true))
        print(f"layer {l}: worst gap of the device's choice to the float64 maximum {gap.max():.3e}")
        assert (gap <= 1e-5).all()
        assert ((args[l] == -1) == (np.diff(f["block"][l + 1][0]) == 0)[:, None]).all()
    for l in range(len(net.W_s)):
        for got, r, nm in ((net.dW_s[l], p64["W_s"][l].grad, f"dW_s{l}"), (net.dW_n[l], p64["W_n"][l].grad, f"dW_n{l}"),
                           (net.db[l], p64["b"][l].grad, f"db{l}")):
            got, r = host(got), r.numpy()
            err = np.abs(got - r).max()
            print(f"{nm}: err {err:.3e}, scale {np.abs(r).max():.3e}")
            assert np.abs(r).max() > 0
            assert err <= 2e-5 * max(np.abs(r).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(r).max():.3e}"
    for p, q in zip([p for k in names for p in getattr(net, k)], before):   # lr = 0: the parameters keep their bits
        assert torch.equal(p, q)


def schedule():
    rng = np.random.default_rng(12)
    return [rng.permutation(N)[:128] for _ in range(20)]


@pytest.mark.parametrize("aggr", AGGRS)
def test_batch_steps_lower_the_full_graph_loss_and_repeat(env, task, aggr):
    torch, g = env["torch"], task["g"]
    X, t = task["dX"], task["dtarget"]
    runs = []
    for _ in range(2):
        net = make_net(env, g, aggr)
        before = float(host(net.evaluate(X, t, task["all_rows"])[0])[0])
        losses = [float(host(net.batch_step(X, t, g.sampled_field(dev(env, b), [5, 5], seed=it), lr=LR))[0]) for it, b in enumerate(schedule())]
        after = float(host(net.evaluate(X, t, task["all_rows"])[0])[0])
        assert all(np.isfinite(losses)) and after < before, (before, after)
        runs.append((losses, after, [p.clone() for p in params(net)]))
    print(f"{aggr}: full-graph loss {before:.4f} -> {after:.4f}; batch loss {runs[0][0][0]:.4f} -> {runs[0][0][-1]:.4f}")
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for p, q in zip(runs[0][2], runs[1][2]):
        assert torch.equal(p, q)


def test_adam_steps_through_batch_step(env, task):
    torch, ops, g = env["torch"], env["ops"], task["g"]
    net = make_net(env, g, "mean").set_optimizer(ops.Adam())
    view = net.on_graph(g.sample_neighbors(5, 0))              # a view made before the steps shares parameters and optimiser
    before = [p.clone() for p in params(net)]
    field = g.sampled_field(dev(env, SEEDS8), [5, 5], seed=0)
    net.batch_step(task["dX"], task["dtarget"], field, lr=0.01)
    view.batch_step(task["dX"], task["dtarget"], field, lr=0.01)
    assert net.optimizer is view.optimizer and net.optimizer.state()["t"] == 2
    assert all(not torch.equal(p, q) for p, q in zip(params(net), before))
    assert all(p is q for p, q in zip(params(net), params(view)))
    plain = make_net(env, g, "mean")
    plain.batch_step(task["dX"], task["dtarget"], field, lr=0.01)
    assert not torch.equal(plain.W_s[0], net.W_s[0])           # Adam's step is not SGD's


def test_refusals(env, task):
    ops, capi = env["ops"], env["capi"]
    moved = ops.CsrGraph.from_coo(dev(env, task["src"]), dev(env, task["dst"]), N, relabel="scramble")
    field = moved.sampled_field(dev(env, SEEDS8), [5, 5], seed=0)        # the field itself is fine on a relabelled graph (mean)
    assert np.array_equal(host(field.query_rows), host(moved.nid)[SEEDS8])
    net = make_net(env, moved, "mean")
    assert net.predict(moved.to_new_order(task["dX"]).contiguous(), field).shape == (8, DIMS[-1])
    with pytest.raises(capi.GnnxError, match="relabel") as info:
        field.map_t(2)
    assert info.value.status == -7
    with pytest.raises(capi.GnnxError, match="relabel"):
        make_net(env, moved, "max")
    net = make_net(env, task["g"], "mean")
    three = task["g"].sampled_field(dev(env, SEEDS8), [5, 5, 5], seed=0)
    with pytest.raises(ValueError):
        net.predict(task["dX"], three)
    with pytest.raises(ValueError):
        net.predict(task["dX"], task["g"].receptive_field(dev(env, SEEDS8), 2))
    with pytest.raises(ValueError):
        net.predict(task["dX"], task["g"].sampled_field(dev(env, SEEDS8[:0]), [5, 5], seed=0))
