"""A NumPy / CPU torch float64 restatement of mini-batch GraphSAGE on a sampled field (ops.SampledField, SageStack.predict /
batch_step), independent of the kernels.  The field is restated from tests/sample_ref.py: block row x of layer l is row rows[l][x] of
the whole-graph sample of (fanouts[l - 1], seeds[l - 1]); Q_{l-1} is Q_l united with the kept columns; columns become positions in
rows[l - 1]; the transposed block is the COO (column, list position) sorted by (column, position).  `forward64` is the float64 model on
the blocks (mean, or max with the winners given or found), `loss64` the loss kernel's form of softmax cross-entropy over all compact
rows of rows[L].  tests/test_minibatch_ref_cpu.py pins all of it to a dense full-graph model and to torch.autograd."""
import numpy as np

from tests.sample_ref import sample_row


def layer_seeds(seed, L):
    """An int s gives layer l (1 .. L) the seed s * L + (l - 1); a sequence is taken as it is."""
    if isinstance(seed, (list, tuple)):
        assert len(seed) == L
        return [int(s) for s in seed]
    return [int(seed) * L + l for l in range(L)]


def sample_rows_ref(rowptr, colidx, rows, k, seed):
    """(rowptr', colidx' with ORIGINAL columns, pos, rowid = list position) of the listed rows, any order, repeats allowed."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx)
    pos, rowid, lens = [], [], []
    for x, i in enumerate(np.asarray(rows, dtype=np.int64)):
        b, d = rowptr[i], int(rowptr[i + 1] - rowptr[i])
        j = sample_row(seed, int(i), d, k)
        pos.append(b + j)
        rowid.append(np.full(len(j), x, dtype=np.int64))
        lens.append(len(j))
    pos = np.concatenate(pos).astype(np.int64) if lens else np.zeros(0, dtype=np.int64)
    rowid = np.concatenate(rowid) if lens else np.zeros(0, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rp, colidx[pos].astype(np.int32), pos.astype(np.int32), rowid.astype(np.int32)


def field_ref(rowptr, colidx, seed_rows, fanouts, seed):
    """The sampled field of the seeds' ROWS (nid already applied) as a dict of lists indexed by layer, entries 1 .. L (rows: 0 .. L):
    rows, nnz, block (rowptr, colidx), self_pos, inv_deg (float32), block_t (rowptr_t, colidx_t), and query_pos."""
    n, L = len(rowptr) - 1, len(fanouts)
    seeds = layer_seeds(seed, L)
    seed_rows = np.asarray(seed_rows, dtype=np.int64)
    f = dict(rows=[None] * (L + 1), nnz=[0] * (L + 1), block=[None] * (L + 1), self_pos=[None] * (L + 1), inv_deg=[None] * (L + 1),
             block_t=[None] * (L + 1), seeds=seeds)
    f["rows"][L] = np.unique(seed_rows).astype(np.int32)
    f["query_pos"] = np.searchsorted(f["rows"][L], seed_rows).astype(np.int32)
    for l in range(L, 0, -1):
        rows_l = f["rows"][l]
        rp, ci, _, rowid = sample_rows_ref(rowptr, colidx, rows_l, fanouts[l - 1], seeds[l - 1])
        below = np.union1d(rows_l, ci).astype(np.int32)
        pos = np.full(n, -1, dtype=np.int32)
        pos[below] = np.arange(len(below), dtype=np.int32)
        ci = pos[ci]
        d = np.diff(rp)
        order = np.argsort(ci.astype(np.int64) * max(len(below), 1) + rowid, kind="stable")
        rpt = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=len(below)))]).astype(np.int32)
        f["rows"][l - 1], f["nnz"][l], f["block"][l] = below, int(rp[-1]), (rp, ci)
        f["self_pos"][l] = pos[rows_l]
        f["inv_deg"][l] = np.where(d > 0, np.float32(1) / np.maximum(d, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        f["block_t"][l] = (rpt, rowid[order].astype(np.int32))
    return f


def row_of_entries(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def forward64(torch, f, X, params, aggr, args=None):
    """Float64 logits on rows[L] (compact) of the model with params = dict(W_s, W_n, b) of float64 torch tensors; X: the full input.
    aggr="max": args[l] (layer index 0 .. L-1, int [|Q_{l+1}|, F], absolute entry positions of the block, -1 for an empty row) names
    the winners; None: the float64 maximum's own (first) winners.  -> (logits, per max layer (float64 maximum, the chosen value))."""
    L = len(params["W_s"])
    h = torch.as_tensor(np.asarray(X, dtype=np.float64))[torch.from_numpy(f["rows"][0].astype(np.int64))]
    chosen = []
    for l in range(L):
        rp, ci = f["block"][l + 1]
        m, F = len(rp) - 1, h.shape[1]
        rows_e = torch.from_numpy(row_of_entries(rp))
        cols_e = torch.from_numpy(ci.astype(np.int64))
        if aggr == "mean":
            inv = torch.from_numpy(np.where(np.diff(rp) > 0, 1.0 / np.maximum(np.diff(rp), 1), 0.0))
            M = torch.zeros((m, F), dtype=torch.float64).index_add(0, rows_e, h[cols_e]) * inv[:, None]
        else:
            true = torch.zeros((m, F), dtype=torch.float64).scatter_reduce(0, rows_e[:, None].expand(-1, F), h.detach()[cols_e], "amax",
                                                                           include_self=False)
            if args is None:
                a = np.full((m, F), -1, dtype=np.int64)
                hv = h.detach().numpy()
                for i in range(m):
                    if rp[i + 1] > rp[i]:
                        a[i] = rp[i] + np.argmax(hv[ci[rp[i]:rp[i + 1]]], axis=0)
                a = torch.from_numpy(a)
            else:
                a = torch.from_numpy(np.asarray(args[l]).astype(np.int64))
            cols_pad = torch.cat([cols_e, torch.zeros(1, dtype=torch.int64)])      # -1 picks the pad
            M = torch.where(a >= 0, h.gather(0, cols_pad[a]), torch.zeros((), dtype=torch.float64))
            chosen.append((true.numpy(), M.detach().numpy()))
        own = h[torch.from_numpy(f["self_pos"][l + 1].astype(np.int64))]
        Z = own @ params["W_s"][l].T + M @ params["W_n"][l].T + params["b"][l]
        h = torch.relu(Z) if l + 1 < L else Z
    return h, chosen


def loss64(torch, logits, target_rows):
    """Mean softmax cross-entropy over all rows of `logits`, in the loss kernel's form; target_rows: the targets of those rows."""
    tgt = torch.from_numpy(np.asarray(target_rows).astype(np.int64))
    picked = logits[torch.arange(logits.shape[0]), tgt]
    return (-torch.log(torch.exp(picked) / (torch.exp(logits).sum(1) + 1e-20))).sum() / logits.shape[0]


def backward64(f, X, W_s, W_n, b, aggr, target_rows):
    """A hand-written float64 forward / loss / backward on the blocks in NumPy, the way the stack runs it (dh = scatter of G W_s through
    self_pos + the transposed block's aggregation; max through its own first winners): -> (loss, dW_s, dW_n, db) lists.  Pinned to
    torch.autograd by tests/test_minibatch_ref_cpu.py."""
    L = len(W_s)
    h = np.asarray(X, dtype=np.float64)[f["rows"][0]]
    saved = []
    for l in range(L):
        rp, ci = f["block"][l + 1]
        m, F = len(rp) - 1, h.shape[1]
        M, arg = np.zeros((m, F)), np.full((m, F), -1, dtype=np.int64)
        for i in range(m):
            if rp[i + 1] > rp[i]:
                v = h[ci[rp[i]:rp[i + 1]]]
                if aggr == "mean":
                    M[i] = v.sum(0) / (rp[i + 1] - rp[i])
                else:
                    arg[i] = rp[i] + np.argmax(v, axis=0)
                    M[i] = v.max(0)
        own = h[f["self_pos"][l + 1]]
        Z = own @ W_s[l].T + M @ W_n[l].T + b[l]
        Y = np.maximum(Z, 0) if l + 1 < L else Z
        saved.append((h, own, M, arg, Y))
        h = Y
    z = h
    tgt = np.asarray(target_rows, dtype=np.int64)
    p = np.exp(z) / (np.exp(z).sum(1, keepdims=True) + 1e-20)
    loss = -np.log(p[np.arange(len(z)), tgt]).sum() / len(z)
    G = p.copy()
    G[np.arange(len(z)), tgt] -= 1
    G /= len(z)
    dW_s, dW_n, db = [None] * L, [None] * L, [None] * L
    for l in reversed(range(L)):
        h_in, own, M, arg, _ = saved[l]
        db[l], dW_s[l], dW_n[l] = G.sum(0), G.T @ own, G.T @ M
        if l == 0:
            break
        rp, ci = f["block"][l + 1]
        dM, dh = G @ W_n[l], np.zeros_like(h_in)
        np.add.at(dh, f["self_pos"][l + 1], G @ W_s[l])
        for i in range(len(rp) - 1):
            for q in range(rp[i], rp[i + 1]):
                if aggr == "mean":
                    dh[ci[q]] += dM[i] / (rp[i + 1] - rp[i])
                else:
                    dh[ci[q]] += np.where(arg[i] == q, dM[i], 0.0)
        G = np.where(h_in > 0, dh, 0.0)
    return loss, dW_s, dW_n, db
