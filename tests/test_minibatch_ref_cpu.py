"""Pins tests/minibatch_ref.py, the CPU restatement of mini-batch GraphSAGE on a sampled field, to things it does not share code with:
with every fanout at least the largest degree the field is the l-hop closure and the seeds' logits are those of a dense float64
full-graph model (1e-12); its hand-written backward equals torch.autograd on a dense restatement; its blocks are per-row slices of
tests/sample_ref.py's whole-graph sample; self_pos, the renumbering and the transposed block are checked against plain loops."""
import numpy as np
import pytest
import torch

from tests import minibatch_ref as mr
from tests.graph_ref import csr_from_coo_ref
from tests.helpers import synth
from tests.sample_ref import sample_ref

DIMS = [6, 8, 5]
AGGRS = ["mean", "max"]


def graphs():
    out = {}
    src, dst = synth.karate_edges()
    out["karate"] = (34,) + csr_from_coo_ref(src, dst, 34)
    src, dst = synth.uniform_edges(17, 300, 1500)
    out["uniform300"] = (300,) + csr_from_coo_ref(src, dst, 300)
    return out


GRAPHS = graphs()
SEEDS = {"karate": np.array([33, 5, 0, 5, 17]), "uniform300": np.array([299, 7, 150, 7, 0, 42, 211, 3])}


def make_params(seed=3):
    rng = np.random.default_rng(seed)
    L = len(DIMS) - 1
    return dict(W_s=[rng.uniform(-1, 1, (DIMS[l + 1], DIMS[l])) * DIMS[l] ** -0.5 for l in range(L)],
                W_n=[rng.uniform(-1, 1, (DIMS[l + 1], DIMS[l])) * DIMS[l] ** -0.5 for l in range(L)],
                b=[rng.uniform(-0.2, 0.2, DIMS[l + 1]) for l in range(L)])


def dense_logits(n, rowptr, colidx, X, p, aggr):
    """The full-graph model on a dense adjacency, float64, no field."""
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = 1.0
    h = X.astype(np.float64)
    L = len(p["W_s"])
    for l in range(L):
        if aggr == "mean":
            deg = A.sum(1)
            M = (A @ h) * np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)[:, None]
        else:
            M = np.where(A.sum(1)[:, None] > 0, np.where(A[:, :, None] > 0, h[None, :, :], -np.inf).max(1), 0.0)
        Z = h @ p["W_s"][l].T + M @ p["W_n"][l].T + p["b"][l]
        h = np.maximum(Z, 0) if l + 1 < L else Z
    return h


def closure(n, rowptr, colidx, rows):
    nxt = set(int(r) for r in rows)
    for r in rows:
        nxt.update(int(c) for c in colidx[rowptr[r]:rowptr[r + 1]])
    return np.array(sorted(nxt), dtype=np.int32)


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("aggr", AGGRS)
def test_a_wide_fanout_gives_the_closure_and_the_dense_models_logits(name, aggr):
    n, rowptr, colidx = GRAPHS[name]
    k = int(np.diff(rowptr).max())
    f = mr.field_ref(rowptr, colidx, SEEDS[name], [k, k + 3], seed=4)
    rows = np.unique(SEEDS[name]).astype(np.int32)
    assert np.array_equal(f["rows"][2], rows)
    for l in (2, 1):
        rows = closure(n, rowptr, colidx, rows)
        assert np.array_equal(f["rows"][l - 1], rows)
    assert len(f["rows"][0]) < n or name == "karate"
    X = np.random.default_rng(1).uniform(-1, 1, (n, DIMS[0]))
    p = make_params()
    tp = {k_: [torch.from_numpy(w) for w in v] for k_, v in p.items()}
    logits, _ = mr.forward64(torch, f, X, tp, aggr)
    ref = dense_logits(n, rowptr, colidx, X, p, aggr)
    assert np.abs(logits.numpy() - ref[f["rows"][2]]).max() <= 1e-12
    assert np.abs(logits.numpy()[f["query_pos"]] - ref[SEEDS[name]]).max() <= 1e-12


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("aggr", AGGRS)
def test_the_backward_equals_autograd_on_a_dense_restatement(name, aggr):
    n, rowptr, colidx = GRAPHS[name]
    f = mr.field_ref(rowptr, colidx, SEEDS[name], [3, 2], seed=[11, 12])
    X = np.random.default_rng(2).uniform(-1, 1, (n, DIMS[0]))
    target = (7 * np.arange(n) + 3) % DIMS[-1]
    p = make_params()
    loss, dW_s, dW_n, db = mr.backward64(f, X, p["W_s"], p["W_n"], p["b"], aggr, target[f["rows"][2]])
    # dense restatement: per layer a dense [|Q_l|, |Q_{l-1}|] matrix of the block and a dense selector of self_pos
    tp = {k_: [torch.tensor(w, requires_grad=True) for w in v] for k_, v in p.items()}
    h = torch.from_numpy(X[f["rows"][0]])
    for l in range(2):
        rp, ci = f["block"][l + 1]
        m, m_in = len(rp) - 1, len(f["rows"][l])
        B = torch.zeros((m, m_in), dtype=torch.float64)
        B[torch.from_numpy(mr.row_of_entries(rp)), torch.from_numpy(ci.astype(np.int64))] = 1.0
        S = torch.zeros((m, m_in), dtype=torch.float64)
        S[torch.arange(m), torch.from_numpy(f["self_pos"][l + 1].astype(np.int64))] = 1.0
        if aggr == "mean":
            deg = B.sum(1)
            M = (B @ h) * torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))[:, None]
        else:
            M = torch.where(B.sum(1)[:, None] > 0, torch.where(B[:, :, None] > 0, h[None, :, :], -torch.inf).amax(1), 0.0)
        Z = (S @ h) @ tp["W_s"][l].T + M @ tp["W_n"][l].T + tp["b"][l]
        h = torch.relu(Z) if l == 0 else Z
    ref = mr.loss64(torch, h, target[f["rows"][2]])
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-12
    for l in range(2):
        for got, r in ((dW_s[l], tp["W_s"][l].grad), (dW_n[l], tp["W_n"][l].grad), (db[l], tp["b"][l].grad)):
            assert np.abs(r.numpy()).max() > 0
            assert np.abs(got - r.numpy()).max() <= 1e-12
    # and forward64 + autograd agree with the hand-written pass (the form the GPU test uses)
    tq = {k_: [torch.tensor(w, requires_grad=True) for w in v] for k_, v in p.items()}
    logits, _ = mr.forward64(torch, f, X, tq, aggr)
    mr.loss64(torch, logits, target[f["rows"][2]]).backward()
    for l in range(2):
        assert np.abs(dW_n[l] - tq["W_n"][l].grad.numpy()).max() <= 1e-12 and np.abs(dW_s[l] - tq["W_s"][l].grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("name", list(GRAPHS))
def test_blocks_are_row_slices_of_the_whole_graph_sample(name):
    n, rowptr, colidx = GRAPHS[name]
    fan, seed = [3, 2], 5
    f = mr.field_ref(rowptr, colidx, SEEDS[name], fan, seed)
    assert f["seeds"] == [10, 11] == mr.layer_seeds(5, 2) and mr.layer_seeds([4, 9], 2) == [4, 9]
    for l in (2, 1):
        rp_g, ci_g, _, _ = sample_ref(rowptr, colidx, fan[l - 1], f["seeds"][l - 1])
        rp, ci = f["block"][l]
        rows, below = f["rows"][l], f["rows"][l - 1]
        assert len(rp) == len(rows) + 1 and f["nnz"][l] == rp[-1] == len(ci)
        assert set(rows) <= set(below) and (np.diff(below) > 0).all()
        for x, i in enumerate(rows):                       # the renumbering and self_pos against a plain loop
            want = ci_g[rp_g[i]:rp_g[i + 1]]
            got = ci[rp[x]:rp[x + 1]]
            assert len(got) == len(want) == min(fan[l - 1], rowptr[i + 1] - rowptr[i])
            assert [int(below[c]) for c in got] == [int(c) for c in want]
            assert below[f["self_pos"][l][x]] == i
        d = np.diff(rp)
        assert np.array_equal(f["inv_deg"][l], np.where(d > 0, np.float32(1) / np.maximum(d, 1).astype(np.float32), 0).astype(np.float32))
        rpt, cit = f["block_t"][l]                         # the transposed block, entry by entry
        assert len(rpt) == len(below) + 1 and rpt[-1] == rp[-1]
        pairs = sorted((int(c), x) for x in range(len(rows)) for c in ci[rp[x]:rp[x + 1]])
        assert [(c, int(x)) for c in range(len(below)) for x in cit[rpt[c]:rpt[c + 1]]] == pairs


def test_listed_rows_in_any_order_and_repeated():
    n, rowptr, colidx = GRAPHS["uniform300"]
    rows = np.array([250, 3, 3, 299, 0, 250])
    rp, ci, pos, rowid = mr.sample_rows_ref(rowptr, colidx, rows, 2, seed=8)
    rp_g, ci_g, pos_g, _ = sample_ref(rowptr, colidx, 2, 8)
    for x, i in enumerate(rows):
        assert np.array_equal(ci[rp[x]:rp[x + 1]], ci_g[rp_g[i]:rp_g[i + 1]])
        assert np.array_equal(pos[rp[x]:rp[x + 1]], pos_g[rp_g[i]:rp_g[i + 1]])
        assert (rowid[rp[x]:rp[x + 1]] == x).all()
    e = mr.sample_rows_ref(rowptr, colidx, np.zeros(0, dtype=np.int64), 2, seed=8)
    assert e[0].tolist() == [0] and all(len(a) == 0 for a in e[1:])
