"""GPU tests of link training on every stack (run with -m gpu on an MI355X): SageStack, GatStack, Gatv2Stack and GcnStack take
link_scores / link_grad / link_train_step / link_evaluate from ops._Stack, here on an EdgeSet.from_walks -- positives are co-occurrence
pairs of random walks, the unsupervised objective.

Held as tests/test_gpu_link.py holds GcnStack (no bar is new): the pair scores bit for bit against tests/sddmm_ref.py, dZ bit for bit
against the two aggregations of tests/spmm_ref.py, and one whole step against a float64 autograd model of the same stack and decoder
(sddmm_ref.bce_logits_ref64 for the loss and its derivative) at that file's bounds: 1e-5 * max(1, |ref|) for the loss,
2e-5 * max(|ref|_max, 1e-3) for every parameter gradient.  The float64 stacks restate tests/test_gpu_sage.py, test_gpu_gat_heads.py and
test_gpu_gatv2_stack.py's models up to the embeddings."""
import numpy as np
import pytest

from tests import edge_softmax_ref as er
from tests import negative_ref as nr
from tests import sddmm_ref as sr
from tests.helpers import synth
from tests.spmm_ref import spmm_ref
from tests.test_gpu_link import dev, env, host  # noqa: F401  (the fixture and helpers of that file)
from tests.test_gpu_negative import assert_metrics_equal

pytestmark = pytest.mark.gpu

N, E, DIMS, HEADS, SLOPE = 256, 1500, [16, 32, 16], [4, 1], 0.2
KINDS = ["sage", "gat", "gatv2", "gcn"]


@pytest.fixture(scope="module")
def task(env):
    ops = env["ops"]
    src, dst = synth.rmat_edges(91, N, E)
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), N)
    g.make_plans(64, max(DIMS))
    walks = g.random_walk(env["torch"].arange(N, dtype=env["torch"].int32, device=env["dev"]), 5, seed=3)
    edges = ops.EdgeSet.from_walks(g, walks, 2, 1, seed=3)
    target = host(edges.target)
    assert edges.nnz > 1000 and 0 < (target == 0).sum() and (target == 1).sum() > 500
    return dict(g=g, edges=edges, rowptr=host(g.rowptr), colidx=host(g.colidx), norm=host(g.norm), X=synth.uniform_pm1(93, (N, DIMS[0])))


def make_net(env, task, kind, seed=950):
    ops, g = env["ops"], task["g"]
    net = {"sage": lambda: ops.SageStack(g, DIMS, aggr="mean", seed=seed), "gat": lambda: ops.GatStack(g, DIMS, seed=seed, heads=HEADS),
           "gatv2": lambda: ops.Gatv2Stack(g, DIMS, seed=seed, heads=HEADS), "gcn": lambda: ops.GcnStack(g, DIMS, seed=seed)}[kind]()
    for l in range(len(DIMS) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(960 + l, (DIMS[l + 1],), scale=0.2)))
    return net


PARAMS = {"sage": ("W_s", "W_n", "b"), "gat": ("W", "A", "b"), "gatv2": ("W", "a", "b"), "gcn": ("W", "b")}


def embed64(torch, task, kind, P):
    """The stack's embeddings in float64 autograd from float64 copies P of the device's parameters."""
    rows_e = torch.from_numpy(er.row_of_entries(task["rowptr"]))
    cols_e = torch.from_numpy(task["colidx"].astype(np.int64))
    nnz = len(cols_e)
    deg = np.diff(task["rowptr"])
    h = torch.from_numpy(task["X"].astype(np.float64))
    L = len(DIMS) - 1

    def attend(e, V, Hh):      # softmax of the scores over each row, then the per-head aggregation of V
        m = torch.full((N, Hh), -float("inf"), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, Hh), e.detach(), "amax")
        x = torch.exp(e - m[rows_e])
        alpha = x / torch.zeros((N, Hh), dtype=torch.float64).index_add(0, rows_e, x)[rows_e]
        msg = alpha[:, :, None] * V[cols_e].view(nnz, Hh, -1)
        return torch.zeros((N, Hh, msg.shape[2]), dtype=torch.float64).index_add(0, rows_e, msg).reshape(N, -1)

    for l in range(L):
        if kind == "sage":
            inv_deg = torch.from_numpy(np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0))
            M = torch.zeros((N, h.shape[1]), dtype=torch.float64).index_add(0, rows_e, h[cols_e]) * inv_deg[:, None]
            Z = h @ P["W_s"][l].T + M @ P["W_n"][l].T + P["b"][l]
        elif kind == "gat":
            Hh = HEADS[l]
            H = h @ P["W"][l].T
            ER = H @ P["A"][l].T
            Z = attend(torch.nn.functional.leaky_relu(ER[rows_e, :Hh] + ER[cols_e, Hh:], SLOPE32), H, Hh) + P["b"][l]
        elif kind == "gatv2":
            Hh = HEADS[l]
            Hlr = h @ P["W"][l].T
            out = Hlr.shape[1] // 2
            Hl, Hr = Hlr[:, :out], Hlr[:, out:]
            u = torch.nn.functional.leaky_relu(Hl[rows_e] + Hr[cols_e], SLOPE32)
            Z = attend((P["a"][l] * u).view(nnz, Hh, -1).sum(2), Hr, Hh) + P["b"][l]
        else:
            H = h @ P["W"][l].T
            agg = torch.zeros((N, H.shape[1]), dtype=torch.float64).index_add(0, rows_e, H[cols_e])
            Z = torch.from_numpy(task["norm"].astype(np.float64))[:, None] * agg + P["b"][l]
        h = torch.relu(Z) if l + 1 < L else Z
    return h


SLOPE32 = float(np.float32(SLOPE))


@pytest.mark.parametrize("kind", KINDS)
def test_link_scores_and_score_gradient_bits(env, task, kind):
    ops, torch = env["ops"], env["torch"]
    net, e = make_net(env, task, kind), task["edges"]
    X = dev(env, task["X"])
    scores = net.link_scores(X, e)
    Z = net.forward(X)
    Zh = host(Z)
    assert Zh.shape == (N, DIMS[-1])
    rowptr, colidx = host(e.rowptr), host(e.colidx)
    assert np.array_equal(host(scores), sr.sddmm_ref(rowptr, colidx, Zh, Zh))
    loss, ds = ops.bce_logits(scores, e.target)
    dZ = net.link_grad(Z, e, ds)
    dsh = host(ds)
    first = spmm_ref(rowptr, colidx, Zh, vals=dsh)
    ref = spmm_ref(host(e.rowptr_t), host(e.colidx_t), Zh, vals=dsh[host(e.map_t)], y0=first)
    assert np.array_equal(host(dZ), ref)
    assert dZ.data_ptr() == net.grad_buffer().data_ptr()
    assert torch.equal(dZ, net.link_grad(Z, e, ds, out=torch.empty_like(dZ)))


@pytest.mark.parametrize("kind", KINDS)
def test_link_step_vs_float64(env, task, kind):
    """Loss and every parameter gradient of one step against the float64 autograd model of the same stack and decoder."""
    torch = env["torch"]
    net, e = make_net(env, task, kind), task["edges"]
    names = PARAMS[kind]
    before = [p.clone() for p in net.params()]
    P = {k: [torch.tensor(host(p).astype(np.float64), requires_grad=True) for p in getattr(net, k)] for k in names}
    loss = net.link_train_step(dev(env, task["X"]), e, lr=0.0)          # lr = 0: the gradients stay, the parameters do not move
    rows = torch.from_numpy(sr.row_of_entries(host(e.rowptr)).astype(np.int64))
    cols = torch.from_numpy(host(e.colidx).astype(np.int64))
    Z = embed64(torch, task, kind, P)
    s = (Z[rows] * Z[cols]).sum(1)
    loss_ref, gsig = sr.bce_logits_ref64(s.detach().numpy(), host(e.target).astype(np.float64))
    s.backward(torch.from_numpy(gsig / len(s)))
    got_loss = float(host(loss)[0])
    print(f"{kind}: loss {got_loss!r} vs float64 {loss_ref!r}")
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    for k in names:
        for l, (got, p) in enumerate(zip(getattr(net, "d" + k), P[k])):
            got, ref = host(got), p.grad.numpy()
            if k == "A":          # GatStack: the blocks of A are the parameters
                mask = host(net.A_mask[l]) != 0
                assert (got[~mask] == 0).all(), "an entry of dA outside the blocks"
                ref = np.where(mask, ref, 0.0)
            err = np.abs(got - ref).max()
            print(f"d{k}{l}: err {err:.3e}, scale {np.abs(ref).max():.3e}")
            assert np.abs(ref).max() > 0
            assert err <= 2e-5 * max(np.abs(ref).max(), 1e-3), f"d{k}{l}: {err:.3e} vs scale {np.abs(ref).max():.3e}"
    for p, q in zip(net.params(), before):
        assert torch.equal(p, q)


def test_walk_epochs_repeat_bit_for_bit(env, task):
    """Unsupervised epochs as the README writes them -- fresh walks and fresh negatives per epoch -- twice: the same losses, the same
    parameters."""
    torch, ops, g = env["torch"], env["ops"], task["g"]
    X = dev(env, task["X"])
    batch = torch.arange(0, N, 2, dtype=torch.int32, device=env["dev"])
    runs = []
    for _ in range(2):
        net = make_net(env, task, "sage")
        losses = [float(host(net.link_train_step(X, ops.EdgeSet.from_walks(g, g.random_walk(batch, 5, seed=ep), 2, 1, seed=ep), lr=1e-3))[0])
                  for ep in range(5)]
        assert all(np.isfinite(losses)), losses
        runs.append((losses, [p.clone() for p in net.params()]))
    assert runs[0][0] == runs[1][0] and len(set(runs[0][0])) == 5
    for p, q in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p, q)


def test_link_evaluate_on_sage_is_the_composition(env, task):
    """link_evaluate = the reference metrics of sddmm_ref scores on the positives and on their reference draws, as
    tests/test_gpu_negative.py holds GcnStack's."""
    rowptr, colidx = task["rowptr"], task["colidx"]
    keep = np.arange(len(colidx)) % 3 == 0                                   # the held-out edges: every third entry
    pos_rowptr = np.concatenate([[0], np.cumsum(np.bincount(sr.row_of_entries(rowptr)[keep], minlength=N))]).astype(np.int32)
    pos_colidx = colidx[keep]
    net = make_net(env, task, "sage")
    X = dev(env, task["X"])
    m, ks = 4, (1, 10, 50)
    got = net.link_evaluate(X, task["g"], (dev(env, pos_rowptr), dev(env, pos_colidx)), m, 77, ks=ks)
    Z = host(net.forward(X))
    neg, unfilled = nr.negatives_ref(pos_rowptr, rowptr, colidx, N, m, 77, 1)
    assert unfilled == 0
    s = sr.sddmm_ref(pos_rowptr, pos_colidx, Z, Z)
    q = sr.sddmm_ref(pos_rowptr * m, neg.reshape(-1), Z, Z).reshape(-1, m)
    assert_metrics_equal(got, nr.metrics_ref(s, q, neg, ks), ks)
