"""GPU tests of the stacks' gradient buffer and its zeroed-rows mark (run with -m gpu on an MI355X): GcnStack, GatStack (heads [2, 1]) and
SageStack (mean, max) on one uniform graph with N = 96 and E = 400, dims [12, 8, 5], every third vertex selected, lr = 0.1.

train_step writes dlogits for the selected rows only (softmax_ce_rows), so the buffer must be zero on every other row; the stack zeroes it
when a selection object is first used and remembers that object.  Bars, all bit for bit:
  (a) a full-row write into net.grad_buffer() between two masked steps (softmax_ce, no backward, no step) changes nothing: both losses and
      every parameter equal those of a net that ran the two steps alone, and the buffer is zero outside the selection afterwards;
  (b) a step with a second selection object over other rows leaves the buffer zero outside THOSE rows and the parameters of the step
      composed by hand with a fresh zero buffer (GcnStack has this in test_gpu_masked.py);
  (c) a SageStack and its on_graph view share the buffer AND the mark: a step through the view, then one through the stack, with the same
      row object, equal plain steps of stacks built on the two graphs; grad_buffer() of the view drops the mark for the stack too."""
import importlib

import numpy as np
import pytest

from tests.helpers import synth

pytestmark = pytest.mark.gpu

N, E, DIMS, HEADS = 96, 400, [12, 8, 5], [2, 1]
LR = 0.1
KINDS = ["gcn", "gat", "sage-mean", "sage-max"]


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


@pytest.fixture(scope="module")
def task(env):
    ops = env["ops"]
    src, dst = synth.uniform_edges(41, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    g2 = g.sample_neighbors(3, seed=5)                       # the same vertices, other neighbourhoods (SageStack.on_graph)
    assert int(g2.nnz) < int(g.nnz)
    X = dev(env, synth.uniform_pm1(43, (N, DIMS[0])))
    target = dev(env, ((7 * np.arange(N) + 3) % DIMS[-1]).astype(np.int32))
    masks = [dev(env, (np.arange(N) % 3 == k).astype(np.uint8)) for k in (0, 1)]     # a third of the rows; a third, other rows
    return dict(g=g, g2=g2, X=X, target=target, masks=masks)


def make_net(env, kind, g):
    ops = env["ops"]
    if kind == "gcn":
        return ops.GcnStack(g, DIMS, seed=7)
    if kind == "gat":
        return ops.GatStack(g, DIMS, seed=7, heads=HEADS)
    return ops.SageStack(g, DIMS, aggr=kind.split("-")[1], seed=7)


def select(kind, g, mask):
    return g.labelled(mask) if kind == "gcn" else g.rows_of(mask)


def params(net):
    name = type(net).__name__
    if name == "GcnStack":
        return net.Wp + net.b
    return net.W + net.A + net.b if name == "GatStack" else net.W_s + net.W_n + net.b


def same_bits(env, a, b):
    torch = env["torch"]
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_same_params(env, a, b, what):
    for k, (p, q) in enumerate(zip(params(a), params(b))):
        assert p.data_ptr() != q.data_ptr() and same_bits(env, p, q), f"{what}: parameter {k}"


def assert_zero_outside(env, net, mask, what):
    """The gradient buffer after a masked step: exactly zero on every row the mask does not select, written on the rows it selects."""
    G = net.grad_buffer()
    assert tuple(G.shape) == (N, DIMS[-1])
    assert bool((G[mask == 0] == 0).all()), f"{what}: a row outside the selection is not zero"
    assert bool((G[mask != 0] != 0).any()), f"{what}: the selected rows were not written"


def write_every_row(env, net, task):
    """softmax_ce over ALL rows into the stack's own buffer: no backward, no step -- the parameters stay."""
    _, d = env["ops"].softmax_ce(net.forward(task["X"]), task["target"], grad_out=net.grad_buffer())
    assert bool((d[task["masks"][1] != 0] != 0).any())       # rows outside the first selection now hold values


@pytest.mark.parametrize("kind", KINDS)
def test_a_full_row_write_between_two_masked_steps_changes_nothing(env, task, kind):
    g, X, t, mask = task["g"], task["X"], task["target"], task["masks"][0]
    sel = select(kind, g, mask)
    A, B = make_net(env, kind, g), make_net(env, kind, g)
    assert_same_params(env, A, B, "before")
    a1 = A.train_step(X, t, sel, LR)
    write_every_row(env, A, task)
    a2 = A.train_step(X, t, sel, LR)
    b1 = B.train_step(X, t, sel, LR)
    b2 = B.train_step(X, t, sel, LR)
    assert same_bits(env, a1, b1), "loss of the first step"
    assert same_bits(env, a2, b2), "loss of the second step"
    assert not same_bits(env, a1, a2)                        # the steps did move the parameters
    assert_same_params(env, A, B, "after the second step")
    assert_zero_outside(env, A, mask, kind)


@pytest.mark.parametrize("kind", KINDS[1:])
def test_a_second_selection_object_gets_a_zeroed_buffer(env, task, kind):
    ops = env["ops"]
    g, X, t = task["g"], task["X"], task["target"]
    sel1, sel2 = (select(kind, g, m) for m in task["masks"])
    net, hand = make_net(env, kind, g), make_net(env, kind, g)
    for n_ in (net, hand):
        n_.train_step(X, t, sel1, LR)
    loss = net.train_step(X, t, sel2, LR)
    # the same step by hand: softmax_ce_rows makes a zero-filled buffer of its own
    loss_h, G = ops.softmax_ce_rows(hand.forward(X), t, sel2, colsum_out=hand.db[-1])
    hand.backward(G, input_grad=False, have_last_bias_grad=True)
    hand.step(LR)
    assert same_bits(env, loss, loss_h)
    assert_same_params(env, net, hand, "after the step on the second selection")
    assert_zero_outside(env, net, task["masks"][1], kind)


@pytest.mark.parametrize("kind", KINDS[2:])
def test_a_sage_view_shares_the_buffer_and_its_mark(env, task, kind):
    g, g2, X, t, mask = task["g"], task["g2"], task["X"], task["target"], task["masks"][0]
    rows = g.rows_of(mask)
    net = make_net(env, kind, g)
    view = net.on_graph(g2)
    l1 = view.train_step(X, t, rows, LR)
    l2 = net.train_step(X, t, rows, LR)
    # two plain steps: a stack built on g2, then a stack built on g that continues from its parameters
    on_g2, on_g = make_net(env, kind, g2), make_net(env, kind, g)
    r1 = on_g2.train_step(X, t, rows, LR)
    for p, q in zip(params(on_g), params(on_g2)):
        p.copy_(q)
    r2 = on_g.train_step(X, t, rows, LR)
    assert same_bits(env, l1, r1) and same_bits(env, l2, r2)
    assert_same_params(env, net, on_g, "a step through the view, one through the stack")
    assert view._buf is net._buf
    # a full-row write through the VIEW's buffer, then a step of the stack with the same row object: zeroed again
    write_every_row(env, view, task)
    l3, r3 = net.train_step(X, t, rows, LR), on_g.train_step(X, t, rows, LR)
    assert same_bits(env, l3, r3)
    assert_same_params(env, net, on_g, "after a full-row write through the view")
    assert_zero_outside(env, net, mask, kind)
    assert view._buf is net._buf
