"""GPU tests of ops.Gatv2Stack (run with -m gpu on an MI355X) on the graph and task of tests/test_gpu_gat_heads.py: R-MAT N = 1024,
E = 8000, once with the diagonal stripped (isolated vertices: empty softmax rows) and once filled, dims [16, 32, 16].

Bars (the project's own for this structure, tests/test_gpu_gat_heads.py): bit equality of one layer against the chain of restatements --
e from the device's own Hl, Hr through tests/gatv2_ref.py, alpha through tests/heads_ref.py with the device's expf, Y through
heads_ref.spmm_heads_ref; one whole step against a float64 autograd model at 1e-5 * max(1, |ref|) for the loss and
2e-5 * max(|ref|_max, 1e-3) for every parameter gradient; heads = [1, 1] against heads = None bit for bit; training goes down and repeats
bit for bit."""
import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import gatv2_ref as gr
from tests import heads_ref as hr
from tests.helpers import synth
from tests.test_gpu_gat_heads import DIMS, LR, N, dev, env, host, task  # noqa: F401  (the fixtures of that file: its graph and task)

pytestmark = pytest.mark.gpu

HEADS = [4, 1]
SLOPE = 0.2


def make_net(env, task, dims=DIMS, heads=HEADS, seed=950, share=False):
    net = env["ops"].Gatv2Stack(task["g"], dims, seed=seed, heads=heads, share_weights=share)
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (dims[l + 1],), scale=0.2)))
    return net


def test_parameters_are_drawn_like_gatstacks(env, task):
    net, shared = make_net(env, task), make_net(env, task, share=True)
    for l, Hh in enumerate(HEADS):
        fan_in, out = DIMS[l], DIMS[l + 1]
        assert tuple(net.W[l].shape) == (2 * out, fan_in) and tuple(shared.W[l].shape) == (out, fan_in) and tuple(net.a[l].shape) == (out,)
        draw = env["ops"].uniform_pm1   # GatStack's generator, seeds and scales: fan_in^-0.5 for the weights, D^-0.5 for a
        assert env["torch"].equal(net.W[l], draw(950 + 2 * l, (2 * out, fan_in), scale=fan_in ** -0.5))
        assert env["torch"].equal(shared.W[l], draw(950 + 2 * l, (out, fan_in), scale=fan_in ** -0.5))
        assert env["torch"].equal(net.a[l], draw(950 + 2 * l + 1, (out,), scale=(out // Hh) ** -0.5))
        assert net.W_l(l).data_ptr() == net.W[l].data_ptr() and net.W_r(l).data_ptr() == net.W[l][out:].data_ptr()
        assert shared.W_l(l) is shared.W[l] and shared.W_r(l) is shared.W[l]
    assert len(net.params()) == len(net.grads()) == 6


@pytest.mark.parametrize("share", [False, True])
def test_one_layer_forward_bits(env, task, share):
    ops = env["ops"]
    Hh, out = 4, DIMS[1]
    net = make_net(env, task, dims=DIMS[:2], heads=[Hh], share=share)
    Y = net.forward(dev(env, task["X"]))
    _, Hlr, e, alpha, _ = net._saved[0]
    nnz = len(task["colidx"])
    assert tuple(Hlr.shape) == (N, out if share else 2 * out) and tuple(e.shape) == (nnz, Hh) and tuple(alpha.shape) == (nnz, Hh)
    Hl, Hr = (host(Hlr), host(Hlr)) if share else (host(Hlr)[:, :out], host(Hlr)[:, out:])
    rp, ci, g = task["rowptr"], task["colidx"], task["g"]
    e_ref = gr.scores_ref(rp, ci, Hl, Hr, host(net.a[0]), Hh, SLOPE)
    assert np.array_equal(host(e), e_ref)
    x_d, m_d, z_d = ops.edge_softmax_heads(g.rowptr, g.colidx, Hh, scores=e, negative_slope=1.0, unnormalised=True, want_stats=True)
    arg, m = hr.exp_argument_heads(er.leaky(hr.pre_activation_heads(rp, ci, scores=e_ref), 1.0), rp)
    assert np.array_equal(host(m_d), m)
    x = host(x_d)
    x64 = np.exp(arg.astype(np.float64))
    normal = x64 >= 2.0 ** -126
    assert (np.abs(x - x64)[normal] <= 2 * np.spacing(x64[normal].astype(np.float32))).all()
    z = hr.row_sum_in_order_heads(x, rp)
    assert np.array_equal(host(z_d), z)
    alpha_ref = hr.edge_softmax_heads_from_x(x, z, rp)
    assert np.array_equal(host(alpha), alpha_ref)
    assert np.array_equal(host(Y), hr.spmm_heads_ref(rp, ci, Hr, alpha_ref, Hh, bias=host(net.b[0])))
    if task["kind"] == "stripped":   # an isolated vertex: the bias alone
        iso = np.nonzero(np.diff(rp) == 0)[0]
        assert len(iso) and np.array_equal(host(Y)[iso], np.broadcast_to(host(net.b[0]), (len(iso), out)))


def model64(torch, task, params, heads, slope, share):
    """GATv2 and its loss in float64 autograd from float64 copies of the device's parameters (W the stacked [W_l; W_r], or the shared one)."""
    rows_e = torch.from_numpy(er.row_of_entries(task["rowptr"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    nnz = len(cols_e)
    h = torch.from_numpy(task["X"].astype(np.float64))
    L = len(params["W"])
    for l in range(L):
        Hh = heads[l]
        Hlr = h @ params["W"][l].T
        out = Hlr.shape[1] if share else Hlr.shape[1] // 2
        Hl, Hr = (Hlr, Hlr) if share else (Hlr[:, :out], Hlr[:, out:])
        u = torch.nn.functional.leaky_relu(Hl[rows_e] + Hr[cols_e], slope)
        e = (params["a"][l] * u).view(nnz, Hh, -1).sum(2)
        m = torch.full((N, Hh), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, Hh), e.detach(), "amax")
        x = torch.exp(e - m[rows_e])
        alpha = x / torch.zeros((N, Hh), dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        msg = alpha[:, :, None] * Hr[cols_e].view(nnz, Hh, -1)
        Y = torch.zeros((N, Hh, msg.shape[2]), dtype=torch.float64).index_add(0, rows_e, msg).reshape(N, -1) + params["b"][l]
        h = torch.relu(Y) if l + 1 < L else Y
    r = torch.from_numpy(task["rows"].astype(np.int64))
    tgt = torch.from_numpy(task["target"].astype(np.int64))[r]
    z = h[r]
    picked = z[torch.arange(len(r)), tgt]
    return (-torch.log(torch.exp(picked) / (torch.exp(z).sum(1) + 1e-20))).sum() / len(r)   # the loss kernel's form


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("heads", [HEADS, None])
def test_one_step_vs_float64(env, task, heads, share):
    torch = env["torch"]
    net = make_net(env, task, heads=heads, share=share)
    before = [p.clone() for p in net.params()]
    params = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in ("W", "a", "b")}
    loss = net.train_step(dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"]), lr=0.0)
    ref = model64(torch, task, params, net.heads, float(np.float32(SLOPE)), share)
    ref.backward()
    got_loss, loss_ref = float(host(loss)[0]), float(ref.detach())
    print(f"loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for l in range(len(net.W)):
        out = DIMS[l + 1]
        dW, dW_ref = host(net.dW[l]), params["W"][l].grad.numpy()
        weights = [(dW, dW_ref, f"dW{l}")] if share else [(dW[:out], dW_ref[:out], f"dW_l{l}"), (dW[out:], dW_ref[out:], f"dW_r{l}")]
        for got, r, nm in weights + [(host(net.da[l]), params["a"][l].grad.numpy(), f"da{l}"), (host(net.db[l]), params["b"][l].grad.numpy(), f"db{l}")]:
            err = np.abs(got - r).max()
            print(f"{nm}: err {err:.3e}, scale {np.abs(r).max():.3e}")
            assert np.abs(r).max() > 0
            assert err <= 2e-5 * max(np.abs(r).max(), 1e-3), f"{nm}: {err:.3e} vs scale {np.abs(r).max():.3e}"
    for p, q in zip(net.params(), before):   # lr = 0: the parameters keep their bits
        assert torch.equal(p, q)


@pytest.mark.parametrize("share", [False, True])
def test_single_heads_equal_no_heads_bit_for_bit(env, task, share):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    one, none = make_net(env, task, heads=[1, 1], share=share), make_net(env, task, heads=None, share=share)
    for p, q in zip(one.params(), none.params()):
        assert torch.equal(p, q)
    assert torch.equal(one.train_step(X, t, rows, lr=0.0), none.train_step(X, t, rows, lr=0.0))
    for p, q in zip(one.grads(), none.grads()):
        assert torch.equal(p, q)
    for _ in range(5):
        assert torch.equal(one.train_step(X, t, rows, lr=LR), none.train_step(X, t, rows, lr=LR))
    for p, q in zip(one.params(), none.params()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("share", [False, True])
def test_training_goes_down_and_repeats_bit_for_bit(env, task, share):
    torch = env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    runs = []
    for _ in range(2):
        net = make_net(env, task, share=share)
        losses = [float(host(net.train_step(X, t, rows, lr=LR))[0]) for _ in range(30)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
        runs.append((losses, [p.clone() for p in net.params()]))
    print(f"loss {runs[0][0][0]:.4f} -> {runs[0][0][-1]:.4f}")
    assert runs[0][0] == runs[1][0]
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)
    loss, correct, count = net.evaluate(X, t, rows)
    assert count == len(task["rows"]) and 0 <= correct <= count and np.isfinite(host(loss)[0])


def test_adam_steps_and_stays_finite(env, task):
    ops, torch = env["ops"], env["torch"]
    X, t, rows = dev(env, task["X"]), dev(env, task["target"]), dev(env, task["rows"])
    net = make_net(env, task).set_optimizer(ops.Adam())
    before = [p.clone() for p in net.params()]
    losses = [float(host(net.train_step(X, t, rows, lr=0.01))[0]) for _ in range(5)]
    print("adam losses", losses)
    assert all(np.isfinite(losses))
    for p, q in zip(net.params(), before):
        assert torch.isfinite(p).all() and not torch.equal(p, q)
    state = net.optimizer.state()
    assert len(state["m"]) == len(net.params()) and state["t"] == 5


def test_backward_returns_the_input_gradient(env, task):
    """forward / backward by hand: dX against float64 autograd of sum(logits * G)."""
    torch = env["torch"]
    net = make_net(env, task)
    X = dev(env, task["X"])
    logits = net.forward(X)
    Gh = synth.uniform_pm1(77, (N, DIMS[-1]))
    dX = net.backward(dev(env, Gh))
    params = {k: [torch.tensor(host(p).astype(np.float64)) for p in getattr(net, k)] for k in ("W", "a", "b")}
    x64 = torch.tensor(task["X"].astype(np.float64), requires_grad=True)
    rows_e = torch.from_numpy(er.row_of_entries(task["rowptr"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    h = x64
    for l, Hh in enumerate(net.heads):
        out = DIMS[l + 1]
        Hlr = h @ params["W"][l].T
        Hl, Hr = Hlr[:, :out], Hlr[:, out:]
        e = (params["a"][l] * torch.nn.functional.leaky_relu(Hl[rows_e] + Hr[cols_e], float(np.float32(SLOPE)))).view(len(cols_e), Hh, -1).sum(2)
        x = torch.exp(e - e.max())
        alpha = x / torch.zeros((N, Hh), dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        Y = torch.zeros((N, Hh, out // Hh), dtype=torch.float64).index_add(0, rows_e, alpha[:, :, None] * Hr[cols_e].view(len(cols_e), Hh, -1))
        Y = Y.reshape(N, -1) + params["b"][l]
        h = torch.relu(Y) if l + 1 < len(net.heads) else Y
    assert np.abs(host(logits) - h.detach().numpy()).max() <= 1e-5 * max(1.0, float(h.detach().abs().max()))
    (h * torch.from_numpy(Gh.astype(np.float64))).sum().backward()
    ref = x64.grad.numpy()
    err = np.abs(host(dX) - ref).max()
    print(f"dX: err {err:.3e}, scale {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0 and err <= 2e-5 * max(np.abs(ref).max(), 1e-3)


def test_bad_heads_are_refused(env, task):
    ops = env["ops"]
    for heads in ([4], [4, 1, 1], [3, 1], [4, 0], [4, 1.5]):
        with pytest.raises(ValueError):
            ops.Gatv2Stack(task["g"], DIMS, heads=heads)


def test_two_rows_rank_the_same_columns_in_opposite_order(env):
    """The dynamic-attention case of tests/test_gatv2_ref_cpu.py through the real kernels: h = I, so Hl = W_l^T and Hr = W_r^T are the
    case's L and R.  GatStack on the same graph ranks the two columns alike in both rows, whatever its parameters."""
    ops, torch = env["ops"], env["torch"]
    rp, ci = (dev(env, x) for x in gr.DYNAMIC["pattern"])
    g = ops.CsrGraph(2, rp, ci, rp.clone(), ci.clone())   # the full 2 x 2 pattern is its own transpose
    net = ops.Gatv2Stack(g, [2, 2], negative_slope=0.2)
    net.W[0].copy_(dev(env, np.concatenate([gr.DYNAMIC["L"].T, gr.DYNAMIC["R"].T])))
    net.a[0].copy_(dev(env, gr.DYNAMIC["a"]))
    net.forward(torch.eye(2, dtype=torch.float32, device=env["dev"]))
    _, Hlr, e, alpha, _ = net._saved[0]
    assert np.array_equal(host(Hlr), np.concatenate([gr.DYNAMIC["L"], gr.DYNAMIC["R"]], axis=1))
    assert np.array_equal(host(e), gr.scores_ref(*gr.DYNAMIC["pattern"], gr.DYNAMIC["L"], gr.DYNAMIC["R"], gr.DYNAMIC["a"], 1, 0.2))
    al = host(alpha).reshape(2, 2)
    assert al[0, 0] > al[0, 1] and al[1, 1] > al[1, 0]
    for seed in range(4):
        gat = ops.GatStack(g, [2, 2], seed=seed)
        gat.forward(dev(env, synth.uniform_pm1(40 + seed, (2, 2))))
        al = host(gat._saved[0][3]).reshape(2, 2)
        assert np.sign(al[0, 0] - al[0, 1]) == np.sign(al[1, 0] - al[1, 1])
