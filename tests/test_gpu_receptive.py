"""GPU tests of query inference (run with -m gpu on an MI355X): frontier marking, position tables and row extraction against the numpy
restatement tests/receptive_ref.py (itself held to hand-written expectations by tests/test_receptive_cpu.py), and
GcnStack.predict / evaluate_field against the full forward.

Bars (none is new):
  * index work (frontiers, compact CSR blocks, carried values): array_equal against numpy, every element;
  * predict: BIT equality (torch.equal) with forward(X) on the query's rows -- a compact block keeps every row's stored order and every
    product is one k-ascending fmaf chain per output element; every element of every query, no sampling;
  * independence from the path under test: a chain of oracle.aggregate_fwd (bit-exact aggregation) and float64 products on the golden
    karate and Cora-sized fixtures, |gpu - ref| <= 1e-5 * max(1, |ref|) (tests.helpers.assert_close);
  * evaluate_field: the same correct count and the same loss bits as evaluate on the same rows.
"""
import functools
import importlib
import time

import numpy as np
import pytest

import oracle
from tests.golden_util import case_inputs
from tests.helpers import assert_close, synth
from tests.receptive_ref import ref_extract, ref_field, ref_frontier

pytestmark = pytest.mark.gpu

N_BIG, E_BIG = 1 << 17, 1_500_000
T0 = time.time()


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the gpu-marked tests must run on an MI355X")
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    assert capi.device_count() >= 1
    yield dict(torch=torch, ops=ops, capi=capi, dev=torch.device("cuda:0"))
    print(f"\ntests/test_gpu_receptive.py: {time.time() - T0:.1f} s from import to the last test")


def dev(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def edges(kind):
    return (synth.rmat_edges if kind == "rmat" else synth.uniform_edges)(71, N_BIG, E_BIG)


_graphs = {}


def graph(env, kind, relabel, chunk=0, extra_vertices=0):
    """The ~2^17-vertex graph of a kind, cached per (kind, order, plan chunk); extra_vertices appends isolated vertices."""
    key = (kind, relabel, chunk, extra_vertices)
    if key not in _graphs:
        src, dst = edges(kind)
        g = env["ops"].CsrGraph.from_coo(dev(env, src), dev(env, dst), N_BIG + extra_vertices, transpose=bool(chunk), relabel=relabel)
        if chunk:
            g.make_plans(chunk, 128)
        _graphs[key] = g
    return _graphs[key]


# ------------------------------------------------------------------ 1. marking, positions, extraction against ref_field
def row_lists(rp, n):
    rng = np.random.default_rng(72)
    pick = lambda k: np.sort(rng.permutation(n)[:k]).astype(np.int32)  # noqa: E731
    return [("one", pick(1)), ("63", pick(63)), ("64", pick(64)), ("65", pick(65)), ("1pct", pick(n // 100)),
            ("all", np.arange(n, dtype=np.int32)), ("longest", np.array([int(np.argmax(np.diff(rp)))], dtype=np.int32)),
            ("empty", np.zeros(0, dtype=np.int32))]


@pytest.mark.parametrize("relabel", [None, "scramble"])
@pytest.mark.parametrize("kind", ["uniform", "rmat"])
def test_marking_positions_and_extraction_equal_the_numpy_restatement(env, kind, relabel):
    ops, torch = env["ops"], env["torch"]
    g = graph(env, kind, relabel)
    n = g.n
    rp, ci = host(g.rowptr), host(g.colidx)
    if kind == "rmat":
        assert np.diff(rp).max() > 64 * 20          # rows far above a 64-entry chunk (and above the plan chunk of the stack tests)
    if relabel is not None:                         # stored order is not ascending column order: "kept" is visible in colidx'
        assert np.any(np.diff(ci)[np.setdiff1d(np.arange(len(ci) - 1), rp[1:-1] - 1)] < 0)
    vals = synth.uniform_pm1(73, (len(ci),))
    vals_d = dev(env, vals)
    for name, rows in row_lists(rp, n):
        rows_d = dev(env, rows)
        cols, n_ent = ops._frontier(g.rowptr, g.colidx, rows_d, n)
        ecols, e_ent = ref_frontier(rp, ci, rows)
        assert cols.dtype == torch.int32 and np.array_equal(host(cols), ecols), name
        assert n_ent == e_ent, name
        assert torch.equal(ops.frontier(g.rowptr, g.colidx, rows_d, n), cols)
        pos = ops.rows_to_positions(cols, n)
        epos = np.full(n, -1, dtype=np.int32)
        epos[ecols] = np.arange(len(ecols), dtype=np.int32)
        assert np.array_equal(host(pos), epos), name
        for col_pos, col_set in ((pos, ecols), (None, None)):
            for with_vals in (True, False):
                rp2, ci2, v2 = ops.csr_extract_rows(g.rowptr, g.colidx, rows_d, vals=vals_d if with_vals else None, col_pos=col_pos, n_cols=n)
                erp, eci, ev = ref_extract(rp, ci, rows, col_set=col_set, vals=vals if with_vals else None)
                assert rp2.dtype == torch.int32 and np.array_equal(host(rp2), erp), name
                assert int(ci2.numel()) == e_ent and np.array_equal(host(ci2), eci), name
                assert (v2 is None) == (not with_vals)
                if with_vals:
                    assert np.array_equal(host(v2), ev), name
        # the capacity the field build passes (the marking's count) is accepted as it is
        rp3, ci3, _ = ops.csr_extract_rows(g.rowptr, g.colidx, rows_d, col_pos=pos, n_cols=n, nnz_capacity=n_ent)
        erp, eci, _ = ref_extract(rp, ci, rows, col_set=ecols)
        assert np.array_equal(host(rp3), erp) and np.array_equal(host(ci3), eci), name


@pytest.mark.parametrize("relabel", [None, "scramble"])
def test_receptive_field_sets_and_blocks_equal_ref_field(env, relabel):
    ops = env["ops"]
    g = graph(env, "rmat", relabel)
    n = g.n
    rp, ci = host(g.rowptr), host(g.colidx)
    nid = np.arange(n) if g.nid is None else host(g.nid).astype(np.int64)
    rng = np.random.default_rng(74)
    deg_v = np.diff(rp)[nid]
    for name, q, L in (("one", rng.integers(0, n, 1), 3), ("hub", np.array([int(np.argmax(deg_v))]), 2),
                       ("1pct", rng.permutation(n)[:n // 100], 2), ("repeats", np.array([5, 3, 5, 99_999, 3, 0]), 3)):
        f = g.receptive_field(dev(env, q.astype(np.int64)), L)
        e = ref_field(rp, ci, nid[q], L)
        assert f.n_query == len(q) and f.n_layers == L
        assert np.array_equal(host(f.query_rows), nid[q].astype(np.int32)) and np.array_equal(host(f.query_pos), e["query_pos"]), name
        assert list(f.nnz) == e["nnz"], name
        for l in range(L + 1):
            assert np.array_equal(host(f.rows[l]), e["rows"][l]), (name, l)
        for l in range(1, L + 1):
            assert np.array_equal(host(f.block[l][0]), e["blocks"][l][0]) and np.array_equal(host(f.block[l][1]), e["blocks"][l][1]), (name, l)
            assert np.array_equal(host(f.norm[l]), host(g.norm)[e["rows"][l]]), (name, l)
            assert f.plan[l] is None


def test_refusals(env):
    """A column outside the position table's set, a too small capacity, a row list that is not ascending and unique, a column id
    outside [0, n_cols): errors with the stated codes, never a wrong index or a truncated CSR."""
    ops, capi, torch = env["ops"], env["capi"], env["torch"]
    g = graph(env, "rmat", None)
    n = g.n
    rp = host(g.rowptr)
    rows = np.sort(np.argsort(-np.diff(rp))[:3]).astype(np.int32)      # the three longest rows
    rows_d = dev(env, rows)
    cols, n_ent = ops._frontier(g.rowptr, g.colidx, rows_d, n)
    assert n_ent > 3 * 64
    pos = ops.rows_to_positions(cols[:-1], n)                          # the set without its last column
    with pytest.raises(capi.GnnxError) as ei:
        ops.csr_extract_rows(g.rowptr, g.colidx, rows_d, col_pos=pos, n_cols=n)
    assert ei.value.status == -3                                       # GNNX_ERR_INDEX_RANGE
    with pytest.raises(capi.GnnxError) as ei:
        ops.csr_extract_rows(g.rowptr, g.colidx, rows_d, n_cols=n, nnz_capacity=n_ent - 1)
    assert ei.value.status == -1 and "nnz_capacity" in str(ei.value)
    for bad in (rows[::-1].copy(), np.array([rows[0], rows[0]], dtype=np.int32), np.array([-1], dtype=np.int32),
                np.array([n], dtype=np.int32)):
        for call in (lambda r: ops.frontier(g.rowptr, g.colidx, r, n), lambda r: ops.csr_extract_rows(g.rowptr, g.colidx, r, nnz_capacity=g.nnz),
                     lambda r: ops.rows_to_positions(r, n)):
            with pytest.raises(capi.GnnxError) as ei:
                call(dev(env, bad))
            assert ei.value.status == -3
    small = int(host(cols)[-1])                                        # the largest stored column is outside [0, small)
    with pytest.raises(capi.GnnxError) as ei:
        ops.frontier(g.rowptr, g.colidx, rows_d, small)
    assert ei.value.status == -3
    with pytest.raises(capi.GnnxError) as ei:
        ops.csr_extract_rows(g.rowptr, g.colidx, rows_d, n_cols=small, nnz_capacity=n_ent)
    assert ei.value.status == -3
    with pytest.raises(ValueError):
        g.receptive_field(torch.tensor([0, n], device="cuda"), 2)      # a vertex id outside the graph
    with pytest.raises(ValueError):
        g.receptive_field(torch.tensor([0.5], device="cuda"), 2)


# ------------------------------------------------------------------ 2. the headline property
def stack_dims(base, L):
    return [base[0]] + [base[1]] * (L - 1) + [base[-1]]


def make_net(env, g, dims, pad):
    ops = env["ops"]
    net = ops.GcnStack(g, dims, seed=710, pad_streamed=pad)
    assert net.padded == bool(pad)
    for l in range(len(dims) - 1):
        net.b[l].copy_(dev(env, synth.uniform_pm1(720 + l, (dims[l + 1],), scale=0.2)))
    return net


def queries(g, n_real, isolated):
    """(name, vertex ids): one ordinary vertex, the top hub, the appended isolated vertex, 1 % random, every vertex, an unsorted list
    with repeats."""
    rng = np.random.default_rng(75)
    deg_r = host(g.rowptr[1:] - g.rowptr[:-1])
    deg_v = deg_r if g.nid is None else deg_r[host(g.nid).astype(np.int64)]
    hub = int(np.argmax(deg_v))
    ordinary = int(np.nonzero((deg_v > 0) & (deg_v < 64))[0][17])
    few = rng.integers(0, n_real, 40)
    return [("ordinary", np.array([ordinary])), ("hub", np.array([hub])), ("isolated", np.array([isolated])),
            ("1pct", rng.permutation(g.n)[:g.n // 100]), ("all", np.arange(g.n)),
            ("repeats", np.concatenate([few, few[::-3], [hub, isolated, hub]]))], hub


@pytest.mark.parametrize("relabel", [None, "scramble"])
@pytest.mark.parametrize("chunk", [64, 0], ids=["planned", "unplanned"])
@pytest.mark.parametrize("base,pad", [([64, 64, 16], False), ([128, 128, 128], False), ([100, 100, 47], True)], ids=["64-64-16", "128", "100-47-padded"])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_predict_has_the_bits_of_the_full_forward(env, L, base, pad, chunk, relabel):
    ops, torch = env["ops"], env["torch"]
    g = graph(env, "rmat", relabel, chunk=chunk, extra_vertices=1)
    isolated = N_BIG                                                       # the appended vertex: no edge names it
    dims = stack_dims(base, L)
    net = make_net(env, g, dims, pad)
    X = g.to_new_order(dev(env, synth.uniform_pm1(701, (g.n, dims[0]))))
    full = net.forward(X).clone()
    assert bool(torch.isfinite(full).all())
    qs, hub = queries(g, N_BIG, isolated)
    if chunk:
        assert g.plan.n_split_rows > 0                                     # hub kernels on the full side
    for name, q in qs:
        f = g.receptive_field(dev(env, q.astype(np.int64)), L)
        assert f.n_query == len(q) and len(f.rows) == L + 1
        got = net.predict(X, f)
        assert got.shape == (len(q), dims[-1]) and got.is_contiguous()
        want = full[f.query_rows.long()]
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} logits differ"
        if name == "hub" and chunk:
            assert f.plan[L].n_split_rows > 0                              # ... and on the compact side
        if name == "isolated":
            assert [int(r.numel()) for r in f.rows] == [0] * L + [1] and list(f.nnz) == [0] * (L + 1)
            assert torch.equal(got, net.b[-1].reshape(1, -1))              # no neighbours: the last bias
        if name == "all":
            assert int(f.rows[L].numel()) == g.n and f.nnz[L] == g.nnz     # the field is the graph
    with pytest.raises(ValueError):
        net.predict(X, g.receptive_field(dev(env, np.array([hub])), L + 1))


# ------------------------------------------------------------------ 3. independence from the path under test
@pytest.mark.parametrize("name,dims", [("karate_l1", [34, 16, 4]), ("cora_l1", [1433, 16, 7])])
@pytest.mark.parametrize("relabel", [None, "scramble"])
def test_predict_against_an_oracle_chain(env, name, dims, relabel):
    """Reference: H = float64 product rounded to f32, Y = oracle.aggregate_fwd (the bit-exact sequential aggregation), ReLU between
    the layers -- nothing of the GPU path but the weights the stack drew."""
    ops, torch = env["ops"], env["torch"]
    c = case_inputs(name)
    n, src, dst = c["n"], c["src"], c["dst"]
    g = ops.CsrGraph.from_coo(dev(env, src), dev(env, dst), n, transpose=False, relabel=relabel)
    net = make_net(env, g, dims, False)
    rp, ci = oracle.coo_to_csr(src, dst, n)
    _, norm = oracle.degree_norm(rp, ci, n)
    assert np.array_equal(host(g.to_vertex_order(g.norm)), norm)
    X = c["X"]
    h = X
    for l in range(len(dims) - 1):
        H = (h.astype(np.float64) @ host(net.W[l]).astype(np.float64).T).astype(np.float32)
        h = oracle.aggregate_fwd(rp, ci, H, norm, host(net.b[l]))
        if l + 2 < len(dims):
            h = np.maximum(h, 0.0)
    Xd = g.to_new_order(dev(env, X))
    rng = np.random.default_rng(76)
    for q in (np.array([0]), np.array([n - 1, 3, 3, 1]), rng.permutation(n)[:max(n // 10, 2)], np.arange(n)):
        f = g.receptive_field(dev(env, q.astype(np.int64)), len(dims) - 1)
        got = host(net.predict(Xd, f))
        assert_close(got, h[q], f"{name} predict, {len(q)} queries")
    assert int(f.rows[-1].numel()) == n


# ------------------------------------------------------------------ 4. evaluate_field, and predict inside a training step
@pytest.mark.parametrize("relabel", [None, "scramble"])
@pytest.mark.parametrize("base,pad", [([64, 64, 16], False), ([100, 100, 47], True)], ids=["64-64-16", "100-47-padded"])
def test_evaluate_field_equals_evaluate(env, base, pad, relabel):
    ops, torch = env["ops"], env["torch"]
    g = graph(env, "rmat", relabel, chunk=64, extra_vertices=1)
    net = make_net(env, g, base, pad)
    X = g.to_new_order(dev(env, synth.uniform_pm1(701, (g.n, base[0]))))
    top = float(net.forward(X).abs().max())        # the loss has no max-subtraction (like the reference): keep the logits near 8
    assert np.isfinite(top)
    if top > 8.0:
        net.W[-1].mul_(8.0 / top)
    mask = np.zeros(g.n, dtype=np.uint8)
    mask[np.random.default_rng(77).permutation(g.n)[:g.n // 100]] = 1
    t_v = np.where(mask != 0, (7 * np.arange(g.n) + 3) % base[-1], -1).astype(np.int32)
    t = g.to_new_order(dev(env, t_v))
    rows = g.rows_of(dev(env, mask))
    q = np.nonzero(mask)[0]
    f = g.receptive_field(dev(env, np.concatenate([q[::-1], q[:5]]).astype(np.int64)), 2)       # any order, repeats
    assert torch.equal(f.rows[2], rows)
    loss_a, correct_a, count_a = net.evaluate(X, t, rows)
    loss_b, correct_b, count_b = net.evaluate_field(X, t, f)
    print(f"evaluate: loss {float(loss_a):.8g} correct {correct_a}/{count_a}; evaluate_field: loss {float(loss_b):.8g} "
          f"correct {correct_b}/{count_b}")
    assert bool(torch.isfinite(loss_a).all())
    assert torch.equal(loss_a, loss_b) and correct_a == correct_b and count_a == count_b == int(mask.sum())
    # reusable: a second evaluation on the same field (a validation mask evaluated every epoch) gives the same again
    loss_c, correct_c, _ = net.evaluate_field(X, t, f)
    assert torch.equal(loss_c, loss_b) and correct_c == correct_b


@pytest.mark.parametrize("pad", [False, True], ids=["own-widths", "padded"])
def test_predict_between_forward_and_backward_leaves_the_step_intact(env, pad):
    ops, torch = env["ops"], env["torch"]
    g = graph(env, "rmat", "scramble", chunk=64, extra_vertices=1)
    dims = [100, 100, 47] if pad else [64, 64, 16]
    X = g.to_new_order(dev(env, synth.uniform_pm1(701, (g.n, dims[0]))))
    t = dev(env, ((7 * np.arange(g.n) + 3) % dims[-1]).astype(np.int32))
    f = g.receptive_field(dev(env, np.random.default_rng(78).permutation(g.n)[:1000].astype(np.int64)), 2)

    def step(with_predict):
        net = make_net(env, g, dims, pad)
        top = float(net.forward(X).abs().max())
        if top > 8.0:
            net.W[-1].mul_(8.0 / top)
        logits = net.forward(X)
        loss, d = ops.softmax_ce(logits, t, colsum_out=net.db[-1], grad_out=net.grad_buffer())
        pred = net.predict(X, f) if with_predict else None
        if with_predict:
            assert torch.equal(pred, logits[f.query_rows.long()])
        Gin = net.backward(d, have_last_bias_grad=True)
        return dict(logits=logits.clone(), loss=loss.clone(), Gin=Gin.clone(), dW=[w.clone() for w in net.dW], db=[b.clone() for b in net.db])

    a, b = step(False), step(True)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["Gin"], b["Gin"])
    for l in range(len(dims) - 1):
        assert torch.equal(a["dW"][l], b["dW"][l]), f"dW{l}"
        assert torch.equal(a["db"][l], b["db"][l]), f"db{l}"
