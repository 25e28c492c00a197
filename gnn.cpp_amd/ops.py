"""Pointer-level Python driver of the GCN hot path (tests / bench / multi-GPU harness).

torch tensors are used only as owners of device memory and for the current stream; every computation is
a C-ABI call into libgnnx_hip.so (include/gnnx.h).  No CPU fallback exists: a tensor that is not on a
CUDA (HIP) device is an error.

Mirrors the call structure of the reference's GCNConv (src/graph.cpp:170-212):
  CsrGraph.from_coo        <- add_self_loops + edge_to_adj_mat            graph.cpp:172,177
  CsrGraph.s / .norm       <- deg / pow / mm / *=                         graph.cpp:178-185
  linear_fwd               <- Linear::forward                             nn.cpp:205-211
  aggregate_fwd            <- aggregate_and_update (+ bias)               graph.cpp:204-212,188
  aggregate_bwd, colsum,   <- Add/Mul/MatMul/Transpose::_backward         operation.h:114-128,144-167,
  linear_bwd                                                              504-534,416-433
"""
import ctypes as C
import threading

import torch

from . import capi


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise capi.GnnxError(-1, "ops", "tensor is not on a HIP device (there is no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D tensor expected"
    return t.stride(0)


_ws_cache = {}


def _workspace(nbytes, device, tag):
    """Grow-only device scratch buffer per (host thread, device, tag) -- allocated outside the timed/compute calls.
    Per thread because a scratch buffer is only safe to share between calls that are ordered on one stream by one
    submitter (the loopback test runs several ranks as threads of one process)."""
    key = (threading.get_ident(), str(device), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _scratch(query_name, *sizes, device, tag):
    """(scratch, nbytes): the library's own answer to `query_name(*sizes, &nbytes)` and the _workspace of `tag` grown to hold it."""
    nbytes = C.c_size_t(0)
    capi.call(query_name, *sizes, C.byref(nbytes))
    return _workspace(nbytes.value, device, tag), nbytes.value


class SpmmPlan:
    """gnnx_spmm_plan: hub rows (longer than `chunk`) to the sequential hub kernel, non-zero-balanced blocks for the rest; the
    planned aggregation has the same bits as the unplanned one."""

    def __init__(self, rowptr, chunk, max_feat):
        self.h = C.c_void_p()
        self._rowptr = rowptr
        capi.call("gnnx_spmm_plan_create", _ptr(rowptr), rowptr.numel() - 1, int(chunk), int(max_feat),
                  C.byref(self.h), _stream())
        a, b = C.c_int64(0), C.c_int64(0)
        capi.call("gnnx_spmm_plan_info", self.h, C.byref(a), C.byref(b))
        self.n_split_rows, self.n_hub_nnz = a.value, b.value   # hub rows (degree > chunk) and their non-zeros

    def hub_ids_structured(self):
        """gnnx_spmm_plan_hub_ids_structured: the hub rows sit on ids with few one-bits (a synthetic power-law graph as generated)."""
        v = C.c_int(0)
        capi.call("gnnx_spmm_plan_hub_ids_structured", self.h, C.byref(v))
        return bool(v.value)

    def set_big_row_threshold(self, threshold):
        """Hub rows longer than `threshold` take the producer / consumer hub kernel (< 0: the library picks them per call, the
        default; same bits for every value)."""
        capi.call("gnnx_spmm_plan_set_big_row_threshold", self.h, int(threshold))
        return self

    def __del__(self):
        try:
            capi.lib().gnnx_spmm_plan_destroy(self.h)
        except Exception:
            pass


class CsrGraph:
    """CSR of A (forward) and of A^T (backward) with the reference's adjacency semantics, plus s and norm."""

    def __init__(self, n_nodes, rowptr, colidx, rowptr_t=None, colidx_t=None):
        self.n = int(n_nodes)
        self.rowptr, self.colidx = rowptr, colidx
        self.rowptr_t, self.colidx_t = rowptr_t, colidx_t
        self.nnz = int(colidx.numel())
        self.s = self.norm = None
        self.plan = self.plan_t = None
        self.nid = None

    @staticmethod
    def csr_from_coo(src, dst, n_nodes, flags=0):
        """gnnx_csr_from_coo on device int32 tensors -> (rowptr, colidx)."""
        E = int(src.numel())
        dev = src.device
        rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        colidx = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        ws = _workspace(capi.csr_from_coo_workspace(E, n_nodes), dev, "csr")
        nnz = C.c_int64(0)
        capi.call("gnnx_csr_from_coo", _ptr(src), _ptr(dst), E, int(n_nodes), int(flags), _ptr(rowptr), _ptr(colidx),
                  C.byref(nnz), _ptr(ws), ws.numel(), _stream())
        return rowptr, colidx[: nnz.value].clone()

    SCRAMBLE_MUL = 2654435761   # prime above any vertex count: v -> (v * SCRAMBLE_MUL) mod n is a bijection (gnnx_partition_scramble)

    @classmethod
    def from_coo(cls, src, dst, n_nodes, transpose=True, norm=True, relabel=None):
        """relabel: None (vertex v is row v), "scramble" (row nid[v] = (v * SCRAMBLE_MUL) mod n: spreads the hubs of a synthetic
        power-law graph, whose ids have few one-bits, over the cache sets) or an int32 [n] permutation nid.  With a relabelling the
        CSR is built exactly as a one-rank shard is (shard.ShardPlan / gnnx_shard_select_edges + gnnx_halo_plan_create): rows are
        new ids, a row's entries are sorted by ORIGINAL column id -- the reference's summation order -- and only then renumbered,
        so every vertex's result has the same bits as without the relabelling and is stored at row g.nid[v]."""
        if relabel is None:
            rowptr, colidx = cls.csr_from_coo(src, dst, n_nodes)
            g = cls(n_nodes, rowptr, colidx)
            if transpose:
                g.rowptr_t, g.colidx_t = cls.csr_from_coo(dst, src, n_nodes)
            g.nid = None
        else:
            dev = src.device
            if isinstance(relabel, str):
                assert relabel == "scramble"
                nid = ((torch.arange(n_nodes, dtype=torch.int64, device=dev) * cls.SCRAMBLE_MUL) % max(n_nodes, 1)).to(torch.int32)
            else:
                nid = relabel.to(torch.int32)
                if int(nid.numel()) != n_nodes or int(torch.unique(nid).numel()) != n_nodes or int(nid.min()) != 0 or \
                        int(nid.max()) != n_nodes - 1:
                    raise ValueError("relabel must be a permutation of 0..n_nodes-1")
            keep = src != dst                       # self loops are dropped on ORIGINAL ids (rows are renumbered below)
            s_, d_ = src[keep], dst[keep]
            rowptr, ci = cls.csr_from_coo(nid[s_.long()], d_, n_nodes, flags=1)        # flags = 1: keep the diagonal as given
            g = cls(n_nodes, rowptr, nid[ci.long()])
            if transpose:
                rowptr_t, cit = cls.csr_from_coo(nid[d_.long()], s_, n_nodes, flags=1)
                g.rowptr_t, g.colidx_t = rowptr_t, nid[cit.long()]
            g.nid = nid
        if norm:
            g.compute_norm()
        return g

    def to_new_order(self, X):
        """Rows of X (vertex v at row v) in this graph's row order (vertex v at row nid[v])."""
        if self.nid is None:
            return X
        out = torch.empty_like(X)
        out[self.nid.long()] = X
        return out

    def to_vertex_order(self, Y):
        """The inverse: Y has vertex v at row nid[v]; returns it with vertex v at row v."""
        return Y if self.nid is None else Y[self.nid.long()]

    def compute_norm(self):
        dev = self.rowptr.device
        self.s = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.norm = torch.empty(self.n, dtype=torch.float32, device=dev)
        capi.call("gnnx_degree_norm_f32", _ptr(self.rowptr), _ptr(self.colidx), self.n, _ptr(self.s), None,
                  _ptr(self.norm), _stream())
        return self.s, self.norm

    def norm_from_pow_table(self, pow_table):
        """OPT-IN "libm-exact" degree block: s_i = pow_table[1 + deg_i] with the table supplied by the CALLER -- pow_table[k] =
        powf((float)k, -0.5f) evaluated by the host's libm, which is literally what the reference computes (functional.h:253,
        std::pow on the host) -- instead of the device's correctly rounded rsqrt (1 ulp apart for a few degrees >= 1058), then
        norm = (A . s) (.) s through gnnx_degree_norm_f32 with the caller's s (its d_s_cols argument).  Returns (s, norm) in this
        graph's row order; nothing of the graph object changes.  With it the whole chain norm -> aggregation is bit-exact against
        the reference's arithmetic at any size (tests/test_gpu_parity.py::test_headline_config_whole_graph_vs_oracle)."""
        deg1 = (self.rowptr[1:] - self.rowptr[:-1] + 1).long()
        if int(deg1.max()) >= pow_table.numel():
            raise ValueError(f"pow_table has {pow_table.numel()} entries, the largest 1 + degree is {int(deg1.max())}")
        s = pow_table.to(torch.float32)[deg1].contiguous()
        norm = torch.empty(self.n, dtype=torch.float32, device=s.device)
        capi.call("gnnx_degree_norm_f32", _ptr(self.rowptr), _ptr(self.colidx), self.n, None, _ptr(s), _ptr(norm), _stream())
        return s, norm

    def make_plans(self, chunk, max_feat, big_rows=None):
        """Load-balancing plans for power-law rows (forward CSR and transposed CSR).  big_rows: the threshold above which a hub row
        takes the producer / consumer kernel (SpmmPlan.set_big_row_threshold; None = the library's default)."""
        self._plan_args = (int(chunk), int(max_feat), big_rows)   # CsrGraph.labelled builds its plans the same way
        self.plan = SpmmPlan(self.rowptr, chunk, max_feat)
        if self.rowptr_t is not None:
            self.plan_t = SpmmPlan(self.rowptr_t, chunk, max_feat)
        if big_rows is not None:
            for pl in (self.plan, self.plan_t):
                if pl is not None:
                    pl.set_big_row_threshold(big_rows)
        return self.plan, self.plan_t

    def attention_map(self):
        """map_t of this graph (csr_transpose_map, built once and kept): per-entry values of CSR(A) -- attention coefficients, their
        gradients -- move to the order of CSR(A^T) as vals[map_t].  GnnxError on a relabelled graph: its rows store their entries in
        ORIGINAL-id order, not ascending, so the map's binary search has nothing to search (build the graph without `relabel` for an
        attention layer); and on a graph without a transposed CSR."""
        if self.nid is not None:
            raise capi.GnnxError(-7, "attention_map", "a relabelled graph keeps each row in original-id order, not ascending: the "
                                 "transpose map cannot be built on it (build the graph without relabel)")
        if self.rowptr_t is None or self.colidx_t is None:
            raise capi.GnnxError(-1, "attention_map", "the graph has no transposed CSR (from_coo(..., transpose=True))")
        if getattr(self, "_map_t", None) is None:
            self._map_t = csr_transpose_map(self.rowptr, self.colidx, self.rowptr_t, self.colidx_t)
        return self._map_t

    def sample_neighbors(self, k, seed, transpose=True, norm=True):
        """A new CsrGraph on the same vertices whose forward CSR keeps at most k stored neighbours per row (gnnx_csr_sample_neighbors:
        uniform without replacement from `seed`, stored order kept; one seed per epoch).  The transposed CSR is built from the sampled
        COO (column, row) with self loops and duplicates kept -- exactly the sampled entries; s / norm are computed on the sample; plans
        are made the way this graph's were.  GnnxError on a relabelled graph, with attention_map's reasoning: its rows are not
        ascending, and the transposed build would reorder them."""
        if self.nid is not None:
            raise capi.GnnxError(-7, "sample_neighbors", "a relabelled graph keeps each row in original-id order, not ascending: the "
                                 "transposed CSR of a sample cannot be built on it (build the graph without relabel)")
        rowptr, colidx, _, rowid = sample_neighbors(self.rowptr, self.colidx, k, seed, want_rowid=transpose)
        g = CsrGraph(self.n, rowptr, colidx)
        if transpose:
            g.rowptr_t, g.colidx_t = self.csr_from_coo(colidx, rowid, self.n, flags=3)   # keep self loops and duplicates
        if norm:
            g.compute_norm()
        if self.plan is not None:
            g.make_plans(*self._plan_args)
        return g

    def sample_negatives(self, m, seed, positives=None, exclude_self=True):
        """(neg int32 [nnz_pos, m], n_unfilled): m non-neighbours per positive, drawn from the columns its row does not hold in this
        graph's forward CSR (sample_negatives; the row itself excluded too).  positives: an EdgeSet or a (rowptr, colidx) pair on this
        graph's rows -- a training split, held-out edges --, default the graph itself.  GnnxError on a relabelled graph, with
        attention_map's reasoning: its rows are not ascending, and the selection searches them."""
        if self.nid is not None:
            raise capi.GnnxError(-7, "sample_negatives", "a relabelled graph keeps each row in original-id order, not ascending: the "
                                 "selection cannot search it (build the graph without relabel)")
        rowptr, colidx = (self.rowptr, self.colidx) if positives is None else _pattern_of(positives, "sample_negatives")
        if int(rowptr.numel()) != self.n + 1:
            raise capi.GnnxError(-2, "sample_negatives", f"the positives have {int(rowptr.numel()) - 1} rows, the graph {self.n}")
        return sample_negatives(rowptr, m, seed, excluded=(self.rowptr, self.colidx), n_cols=self.n, exclude_self=exclude_self,
                                nnz=None if colidx is None else int(colidx.numel()))

    def random_walk(self, starts, length, seed, p=1.0, q=1.0, walks_per_start=1):
        """int32 [len(starts) * walks_per_start, length + 1]: random walks on this graph's forward CSR (random_walk).  starts: rows of
        this graph (g.nid[v] of vertex ids on a relabelled graph), any order, repeats allowed; walks_per_start repeats the LIST
        block-wise (walk x starts at starts[x % len(starts)]), each repeat an independent walk.  GnnxError on a relabelled graph when
        (p, q) != (1, 1), with attention_map's reasoning: its rows are not ascending, and the second-order step searches the previous
        vertex's row; uniform walks read no order and run on any graph."""
        if self.nid is not None and (float(p), float(q)) != (1.0, 1.0):
            raise capi.GnnxError(-7, "random_walk", "a relabelled graph keeps each row in original-id order, not ascending: the "
                                 "second-order step cannot search it (build the graph without relabel, or walk with p = q = 1)")
        starts = _row_list(starts)
        if int(walks_per_start) != 1:
            starts = starts.repeat(max(int(walks_per_start), 0))
        return random_walk(self.rowptr, self.colidx, starts, length, seed, p, q)

    def mask_in_row_order(self, mask):
        """A vertex-order mask ([n] bool / uint8, vertex v at position v) as uint8 in this graph's row order (vertex v at nid[v])."""
        if int(mask.numel()) != self.n:
            raise ValueError(f"mask has {int(mask.numel())} entries, the graph has {self.n} vertices")
        m = mask.reshape(-1).to(torch.uint8)
        return self.to_new_order(m).contiguous()

    def rows_of(self, mask):
        """The rows of this graph (ascending int32) that hold the vertices of a vertex-order mask."""
        return rows_from_mask(self.mask_in_row_order(mask))

    def labelled(self, mask):
        """The labelled vertex set of semi-supervised training (reference graph.cpp:130-151 set_mask) prepared for the pruned last
        layer: a LabelledSet in this graph's row order.  mask: [n] bool / uint8 in VERTEX order (as X before to_new_order)."""
        return LabelledSet(self, mask)

    def receptive_field(self, query, n_layers):
        """The n_layers-hop receptive field of a vertex set, prepared once for GcnStack.predict / evaluate_field: a ReceptiveField.
        query: 1-D integer tensor of VERTEX ids, any order, repeats allowed."""
        return ReceptiveField(self, query, n_layers)

    def sampled_field(self, seeds, fanouts, seed):
        """The sampled field of one mini-batch for SageStack.predict / batch_step: a SampledField.  seeds: 1-D integer tensor of VERTEX
        ids, any order, repeats allowed; fanouts: neighbours kept per layer, first layer first; seed: an int (one per batch or epoch)
        or one int per layer."""
        return SampledField(self, seeds, fanouts, seed)


class LabelledSet:
    """rows / n_labelled of a train mask, the row-restricted CSR(A) (entries whose row is labelled) and the column-restricted
    CSR(A^T) (entries whose column is labelled, with norm_per_nz_t restricted by the same call), and an SpmmPlan for each when the
    graph has plans (same chunk).  Both CSRs hold the same edge set.  The last layer's aggregations on them have the bits of the
    full ones wherever the loss looks (a dropped term is norm * 0)."""

    def __init__(self, g, mask):
        if g.rowptr_t is None or g.norm is None:
            raise ValueError("labelled() needs the transposed CSR and the norm (from_coo(transpose=True, norm=True))")
        m = g.mask_in_row_order(mask)
        self.mask = m
        self.rows = rows_from_mask(m)
        self.n_labelled = int(self.rows.numel())
        self.rowptr, self.colidx, _ = csr_restrict(g.rowptr, g.colidx, row_keep=m, n_cols=g.n)
        if getattr(g, "norm_per_nz_t", None) is None:
            g.norm_per_nz_t = gather_rows(g.norm.reshape(-1, 1), g.colidx_t).reshape(-1)
        self.rowptr_t, self.colidx_t, self.norm_per_nz_t = csr_restrict(g.rowptr_t, g.colidx_t, vals=g.norm_per_nz_t, col_keep=m, n_cols=g.n)
        self.nnz = int(self.colidx.numel())
        self.plan = self.plan_t = None
        if g.plan is not None:
            chunk, max_feat, big_rows = g._plan_args
            self.plan = SpmmPlan(self.rowptr, chunk, max_feat)
            self.plan_t = SpmmPlan(self.rowptr_t, chunk, max_feat) if g.plan_t is not None else None
            if big_rows is not None:
                for pl in (self.plan, self.plan_t):
                    if pl is not None:
                        pl.set_big_row_threshold(big_rows)


def rows_from_mask(mask):
    """gnnx_mask_to_rows: ascending int32 positions of the non-zero entries of a [n] bool / uint8 device tensor."""
    m = mask.reshape(-1)
    m = (m if m.dtype == torch.uint8 else m.to(torch.uint8)).contiguous()
    n = int(m.numel())
    rows = torch.empty(max(n, 1), dtype=torch.int32, device=m.device)
    ws, _ = _scratch("gnnx_mask_to_rows_workspace", n, device=m.device, tag="mask")
    cnt = C.c_int32(0)
    capi.call("gnnx_mask_to_rows", _ptr(m), n, _ptr(rows), C.byref(cnt), _ptr(ws), ws.numel(), _stream())
    return rows[: cnt.value].clone()


def csr_restrict(rowptr, colidx, vals=None, row_keep=None, col_keep=None, n_cols=None):
    """gnnx_csr_restrict: the CSR with the same rows keeping entry (r, c) iff row_keep[r] (when given) and col_keep[c] (when given);
    stored order inside a row is kept.  Masks: [n_rows] / [n_cols] bool or uint8.  -> (rowptr', colidx', vals' or None)."""
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    dev = rowptr.device
    u8 = lambda t: None if t is None else (t if t.dtype == torch.uint8 else t.to(torch.uint8)).reshape(-1).contiguous()  # noqa: E731
    rk, ck = u8(row_keep), u8(col_keep)
    if rk is not None and int(rk.numel()) != n_rows:
        raise ValueError("row_keep must have one entry per row")
    if n_cols is None:
        n_cols = int(ck.numel()) if ck is not None else n_rows
    if ck is not None and int(ck.numel()) != n_cols:
        raise ValueError("col_keep must have one entry per column")
    rowptr_o = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    colidx_o = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    vals_o = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev) if vals is not None else None
    ws, _ = _scratch("gnnx_csr_restrict_workspace", n_rows, nnz, device=dev, tag="mask")
    out_nnz = C.c_int64(0)
    capi.call("gnnx_csr_restrict", n_rows, int(n_cols), nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(vals), _ptr(rk), _ptr(ck),
              _ptr(rowptr_o), _ptr(colidx_o), _ptr(vals_o), C.byref(out_nnz), _ptr(ws), ws.numel(), _stream())
    k = out_nnz.value
    # (an empty result stays a view of its 1-element buffer: the aggregation wants a device pointer even for no entries)
    shrink = lambda t: None if t is None else (t[:k].clone() if k else t[:0])  # noqa: E731
    return rowptr_o, shrink(colidx_o), shrink(vals_o)


def _row_list(rows):
    r = rows.reshape(-1)
    return (r if r.dtype == torch.int32 else r.to(torch.int32)).contiguous()


def _frontier(rowptr, colidx, rows, n_cols):
    """frontier() and the number of entries of the listed rows (gnnx_frontier_mark's count)"""
    rows = _row_list(rows)
    n_rows, k, dev = int(rowptr.numel() - 1), int(rows.numel()), rowptr.device
    mark = torch.zeros(max(int(n_cols), 1), dtype=torch.uint8, device=dev)
    ws, _ = _scratch("gnnx_frontier_mark_workspace", k, device=dev, tag="field")
    nnz = C.c_int64(0)
    capi.call("gnnx_frontier_mark", _ptr(rowptr), _ptr(colidx) if int(colidx.numel()) else None, n_rows, int(n_cols), _ptr(rows) if k else None, k,
              _ptr(mark), C.byref(nnz), _ptr(ws), ws.numel(), _stream())
    return rows_from_mask(mark[:int(n_cols)]), nnz.value


def frontier(rowptr, colidx, rows, n_cols):
    """gnnx_frontier_mark + gnnx_mask_to_rows: the ascending int32 list of the columns stored in the listed rows (ascending, no
    repeats) of a CSR with n_cols columns -- the rows of the layer below that the listed rows of a layer read."""
    return _frontier(rowptr, colidx, rows, n_cols)[0]


def rows_to_positions(rows, n):
    """gnnx_rows_to_positions: int32 [n], pos[rows[k]] = k and -1 for a row that is not listed."""
    rows = _row_list(rows)
    k, dev = int(rows.numel()), rows.device
    pos = torch.empty(max(int(n), 1), dtype=torch.int32, device=dev)
    ws = _workspace(512, dev, "field_pos")
    capi.call("gnnx_rows_to_positions", _ptr(rows) if k else None, k, int(n), _ptr(pos), _ptr(ws), ws.numel(), _stream())
    return pos[:int(n)]


def csr_extract_rows(rowptr, colidx, rows, vals=None, col_pos=None, n_cols=None, nnz_capacity=None):
    """gnnx_csr_extract_rows: the CSR of the listed rows (ascending, no repeats), entries in stored order, columns renumbered through
    the position table col_pos ([n_cols] int32 from rows_to_positions; None keeps the column ids).  nnz_capacity: entries the outputs
    may hold (default: what the listed rows hold, from rowptr).  -> (rowptr' [len(rows) + 1], colidx', vals' or None)."""
    rows = _row_list(rows)
    n_rows, k, dev = int(rowptr.numel() - 1), int(rows.numel()), rowptr.device
    if n_cols is None:
        n_cols = int(col_pos.numel()) if col_pos is not None else n_rows
    if col_pos is not None and int(col_pos.numel()) != n_cols:
        raise ValueError("col_pos must have one entry per column")
    if nnz_capacity is None:
        r = rows.long()
        nnz_capacity = int((rowptr[r + 1] - rowptr[r]).sum()) if k else 0
    cap = int(nnz_capacity)
    rowptr_o = torch.empty(k + 1, dtype=torch.int32, device=dev)
    colidx_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    vals_o = torch.empty(max(cap, 1), dtype=torch.float32, device=dev) if vals is not None else None
    ws, _ = _scratch("gnnx_csr_extract_rows_workspace", k, device=dev, tag="field")
    out_nnz = C.c_int64(0)
    capi.call("gnnx_csr_extract_rows", n_rows, int(n_cols), _ptr(rowptr), _ptr(colidx) if int(colidx.numel()) else None, _ptr(vals),
              _ptr(rows) if k else None, k, _ptr(col_pos), _ptr(rowptr_o), _ptr(colidx_o), _ptr(vals_o), cap, C.byref(out_nnz), _ptr(ws),
              ws.numel(), _stream())
    m = out_nnz.value
    # (an empty result stays a view of its 1-element buffer, as csr_restrict's: the aggregation wants a device pointer)
    shrink = lambda t: None if t is None else (t[:m] if m else t[:0])  # noqa: E731
    return rowptr_o, shrink(colidx_o), shrink(vals_o)


def sample_neighbors(rowptr, colidx, k, seed, want_pos=False, want_rowid=False):
    """gnnx_csr_sample_neighbors: at most k entries per row, uniformly without replacement from `seed`, kept in stored order.
    -> (rowptr', colidx', pos or None, rowid or None): pos[q] is the absolute position of kept entry q in the input CSR (a per-entry
    array follows the sample as vals[pos]), rowid[q] its row ((colidx', rowid') is the COO of the transposed sample).  The same
    (seed, k) gives the same sample on every run; use one seed per epoch or layer."""
    n_rows, nnz, dev = int(rowptr.numel() - 1), int(colidx.numel()), rowptr.device
    k = int(k)
    ws, _ = _scratch("gnnx_csr_sample_workspace", n_rows, nnz, k, device=dev, tag="sample")   # refuses k < 1 and k > 64 before anything is sized
    cap = int((rowptr[1:] - rowptr[:-1]).clamp(max=k).sum()) if n_rows else 0   # min(deg, k): the capacity is exact
    rowptr_o = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    colidx_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    pos_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if want_pos else None
    rowid_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if want_rowid else None
    out_nnz = C.c_int64(0)
    capi.call("gnnx_csr_sample_neighbors", n_rows, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, k, int(seed) & (2 ** 64 - 1), _ptr(rowptr_o),
              _ptr(colidx_o), _ptr(pos_o), _ptr(rowid_o), cap, C.byref(out_nnz), _ptr(ws), ws.numel(), _stream())
    m = out_nnz.value
    # (an empty result stays a view of its 1-element buffer, as csr_restrict's: the aggregation wants a device pointer)
    shrink = lambda t: None if t is None else (t[:m] if m else t[:0])  # noqa: E731
    return rowptr_o, shrink(colidx_o), shrink(pos_o), shrink(rowid_o)


def sample_rows(rowptr, colidx, rows, k, seed, n_cols=None, want_pos=False, want_rowid=False, col_mark=None):
    """gnnx_csr_sample_rows: sample_neighbors for a list of rows (int32 ids of the CSR, any order, repeats allowed) -- output row x is
    row rows[x] of the whole-graph sample of the same (k, seed), at a cost of O(len(rows) + their entries).
    -> (rowptr' [len(rows) + 1], colidx' (ORIGINAL column ids), pos or None, rowid or None): rowid[q] is the LIST position x of kept entry
    q.  col_mark: a [n_cols] uint8 device tensor in which byte c is set to 1 for every kept column c (zeroed or preset by the caller).
    GnnxError (status -3) with nothing written when the list holds an id outside [0, n_rows)."""
    rows = _row_list(rows)
    n_rows, nnz, m, dev = int(rowptr.numel() - 1), int(colidx.numel()), int(rows.numel()), rowptr.device
    n_cols = n_rows if n_cols is None else int(n_cols)
    k = int(k)
    if col_mark is not None and (col_mark.dtype != torch.uint8 or int(col_mark.numel()) != n_cols or not col_mark.is_contiguous()):
        raise capi.GnnxError(-2, "sample_rows", f"col_mark must be a contiguous uint8 vector of {n_cols} entries")
    ws, _ = _scratch("gnnx_csr_sample_workspace", m, nnz, k, device=dev, tag="sample")   # refuses k < 1 and k > 64 before anything is sized
    cap = 0
    if m and n_rows:   # min(deg, k) of the listed rows: exact (an id outside the CSR is clamped here and refused by the call)
        r = rows.long().clamp(0, n_rows - 1)
        cap = int((rowptr[r + 1] - rowptr[r]).clamp(max=k).sum())
    rowptr_o = torch.empty(m + 1, dtype=torch.int32, device=dev)
    colidx_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    pos_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if want_pos else None
    rowid_o = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if want_rowid else None
    out_nnz = C.c_int64(0)
    capi.call("gnnx_csr_sample_rows", n_rows, n_cols, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(rows) if m else None, m, k,
              int(seed) & (2 ** 64 - 1), _ptr(rowptr_o), _ptr(colidx_o), _ptr(pos_o), _ptr(rowid_o), _ptr(col_mark), cap, C.byref(out_nnz),
              _ptr(ws), ws.numel(), _stream())
    e = out_nnz.value
    # (an empty result stays a view of its 1-element buffer, as csr_restrict's: the aggregation wants a device pointer)
    shrink = lambda t: None if t is None else (t[:e] if e else t[:0])  # noqa: E731
    return rowptr_o, shrink(colidx_o), shrink(pos_o), shrink(rowid_o)


def renumber_cols(colidx, pos):
    """gnnx_csr_renumber_cols: colidx[q] = pos[colidx[q]] IN PLACE (pos: a position table from rows_to_positions).  GnnxError (status
    -3) when a column is outside the table or has no position.  Returns colidx."""
    nnz, n_cols = int(colidx.numel()), int(pos.numel())
    ws = _workspace(256, colidx.device, "renumber")
    capi.call("gnnx_csr_renumber_cols", nnz, _ptr(colidx) if nnz else None, _ptr(pos) if n_cols else None, n_cols, _ptr(ws), ws.numel(), _stream())
    return colidx


NEG_EXCLUDE_SELF = 1


def _pattern_of(positives, where):
    """(rowptr, colidx or None) of a positives argument: an EdgeSet / CsrGraph (its forward pattern) or a (rowptr, colidx) pair."""
    if hasattr(positives, "rowptr") and hasattr(positives, "colidx"):
        return positives.rowptr, positives.colidx
    if isinstance(positives, (tuple, list)) and len(positives) == 2:
        return positives[0], positives[1]
    raise capi.GnnxError(-1, where, "positives: an EdgeSet, a CsrGraph or a (rowptr, colidx) pair expected")


def sample_negatives(rowptr, m, seed, excluded=None, n_cols=None, exclude_self=True, nnz=None):
    """gnnx_csr_sample_negatives: for every entry of the positives pattern `rowptr` (int32 [n_rows + 1]; only the row structure is read;
    nnz = rowptr[-1], read from the device when not given) m columns drawn uniformly from the columns that the entry's row does NOT hold
    in `excluded` = (rowptr_ex, colidx_ex) -- same rows, n_cols columns (default: n_rows), rows strictly ascending; None: nothing is
    excluded -- nor, with exclude_self, the row's own id.  -> (neg int32 [nnz, m], entry-major; n_unfilled): a row that holds every
    column has nothing to draw, its draws are -1 and counted in n_unfilled.  Exact, without a rejection loop; the m draws of a positive
    are independent and may repeat.  The same (seed, m) gives the same draws on every run; use one seed per epoch."""
    n_rows, dev = int(rowptr.numel() - 1), rowptr.device
    n_cols = n_rows if n_cols is None else int(n_cols)
    m = int(m)
    nnz = (int(rowptr[-1]) if n_rows >= 0 and rowptr.numel() else 0) if nnz is None else int(nnz)
    if excluded is None:
        rowptr_ex, colidx_ex = torch.zeros(n_rows + 1, dtype=torch.int32, device=dev), None
    else:
        rowptr_ex, colidx_ex = excluded
        if int(rowptr_ex.numel()) != n_rows + 1:
            raise capi.GnnxError(-2, "sample_negatives", f"the excluded pattern has {int(rowptr_ex.numel()) - 1} rows, the positives {n_rows}")
    nnz_ex = 0 if colidx_ex is None else int(colidx_ex.numel())
    neg = torch.empty((nnz, max(m, 0)), dtype=torch.int32, device=dev)
    ws = _workspace(256, dev, "negatives")
    unfilled = C.c_int64(0)
    capi.call("gnnx_csr_sample_negatives", n_rows, n_cols, nnz, _ptr(rowptr), nnz_ex, _ptr(rowptr_ex), _ptr(colidx_ex) if nnz_ex else None, m,
              int(seed) & (2 ** 64 - 1), NEG_EXCLUDE_SELF if exclude_self else 0, _ptr(neg) if neg.numel() else None, C.byref(unfilled), _ptr(ws),
              ws.numel(), _stream())
    return neg, unfilled.value


def rank_counts(pos_scores, neg_scores, neg=None):
    """gnnx_rank_counts_f32: (greater, equal, valid) int32 [P] for positive scores [P] and negative scores [P, m] (or [P * m],
    entry-major): the number of a positive's negatives that score higher, the same, and that were compared at all.  Draws with
    neg[p, t] < 0 (unfilled, sample_negatives) are skipped; IEEE comparisons: -0 == +0, a NaN on either side counts in none of the
    three, so valid - greater - equal is the number that score lower."""
    P = int(pos_scores.numel())
    if P == 0 or int(neg_scores.numel()) % P:
        if P or int(neg_scores.numel()):
            raise capi.GnnxError(-2, "rank_counts", f"{int(neg_scores.numel())} negative scores for {P} positives")
        m = 1
    else:
        m = int(neg_scores.numel()) // P
    assert pos_scores.is_contiguous() and neg_scores.is_contiguous() and pos_scores.dtype == neg_scores.dtype == torch.float32
    if neg is not None:
        assert neg.is_contiguous() and neg.dtype == torch.int32 and neg.numel() == neg_scores.numel()
    out = torch.empty((3, max(P, 1)), dtype=torch.int32, device=pos_scores.device)
    capi.call("gnnx_rank_counts_f32", P, m, _ptr(pos_scores) if P else None, _ptr(neg_scores) if P else None,
              _ptr(neg) if (neg is not None and P) else None, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
    return out[0, :P], out[1, :P], out[2, :P]


def link_metrics(pos_scores, neg_scores, neg=None, ks=(10, 50, 100)):
    """Ranking metrics of a link model from rank_counts -- integers, so every figure is exact in any summation order.  -> dict:
      mrr           mean of 1 / (1 + greater + equal): the PESSIMISTIC rank (ties rank the positive last), in float64
      hits@K        share of positives with greater + equal < K, for every K of ks
      auc_grouped   (sum(valid - greater - equal) + sum(equal) / 2) / sum(valid): each positive against its own negatives
      auc           the global AUC of all positive scores against all valid negative scores, ties count 1/2 (formed in int64 by a
                    sort and two searches -- plumbing)
      auc_fraction, auc_grouped_fraction   (numerator, denominator) of the two as Python ints, over twice the number of pairs
      n_pos, n_valid   positives, and compared (positive, own negative) pairs
    NaN rule: a NaN score counts as neither above nor below anything.  rank_counts leaves such a comparison out of greater, equal AND
    valid; the global AUC leaves NaN positives and NaN negatives out of numerator and denominator.  A positive without a compared
    negative (a NaN score, a complete row) has rank 1.  A metric whose denominator is 0 is NaN."""
    P = int(pos_scores.numel())
    greater, equal, valid = (t.long() for t in rank_counts(pos_scores, neg_scores, neg))
    ge = greater + equal
    nan = float("nan")
    out = {"n_pos": P, "n_valid": int(valid.sum())}
    out["mrr"] = float((1.0 / (1 + ge).double()).mean()) if P else nan
    for k in ks:
        out[f"hits@{int(k)}"] = int((ge < int(k)).sum()) / P if P else nan
    num, den = int(2 * (valid - ge).sum() + equal.sum()), 2 * out["n_valid"]
    out["auc_grouped_fraction"], out["auc_grouped"] = (num, den), num / den if den else nan
    q = neg_scores.reshape(-1)
    keep = ~q.isnan() if neg is None else (~q.isnan()) & (neg.reshape(-1) >= 0)
    qs, _ = torch.sort(q[keep] + 0.0)          # (+ 0.0: one zero, whatever the sort makes of -0 against +0)
    s = pos_scores.reshape(-1)
    s = s[~s.isnan()] + 0.0
    below = torch.searchsorted(qs, s, right=False)
    upto = torch.searchsorted(qs, s, right=True)
    num, den = int((below + upto).sum()), 2 * int(s.numel()) * int(qs.numel())
    out["auc_fraction"], out["auc"] = (num, den), num / den if den else nan
    return out


def random_walk(rowptr, colidx, starts, length, seed, p=1.0, q=1.0, walk_base=0, out=None):
    """gnnx_csr_random_walk: one walk of `length` steps from every entry of `starts` (int32 row ids of the square CSR, any order, repeats
    allowed) -> int32 [n_walks, length + 1], walk-major: column 0 the start, column t + 1 the result of step t; -1 from the step on
    that left a vertex without neighbours (a start outside the CSR: from column 0 on).  p = q = 1: uniform steps (DeepWalk); otherwise
    node2vec's second-order steps with return parameter p and in-out parameter q, which need strictly ascending rows.  Walk x draws from
    (seed, walk_base + x), never from its start: repeated starts walk independently, and slices of a list with walk_base = the slice's
    offset give the slices of one call.  out: an int32 [n_walks, >= length + 1] row-major tensor or view; columns behind length + 1 are
    not written.  The same arguments give the same walks on every run; use one seed per epoch."""
    starts = _row_list(starts)
    n_rows, nnz, m, L = int(rowptr.numel() - 1), int(colidx.numel()), int(starts.numel()), int(length)
    if out is None:
        out = torch.empty((m, max(L, 0) + 1), dtype=torch.int32, device=rowptr.device)
    elif out.dtype != torch.int32 or out.dim() != 2 or int(out.shape[0]) != m or int(out.shape[1]) < L + 1 or \
            (int(out.shape[1]) > 1 and out.stride(1) != 1):
        raise capi.GnnxError(-2, "random_walk", f"out must be a row-major int32 matrix of {m} rows and at least {L + 1} columns")
    ldw = out.stride(0) if m > 1 else max(int(out.shape[1]), 1)
    capi.call("gnnx_csr_random_walk", n_rows, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(starts) if m else None, m, int(walk_base), L,
              float(p), float(q), int(seed) & (2 ** 64 - 1), _ptr(out) if m else None, ldw, _stream())
    return out[:, :L + 1] if int(out.shape[1]) != L + 1 else out


def walk_pairs(walks, window):
    """The co-occurrence pairs of walks [n_walks, L + 1] within `window` positions -> (src, dst) int32: for every offset o = 1 .. window,
    every position a = 0 .. L - o and every walk x the pair (walks[x, a], walks[x, a + o]) and, straight behind it, its reverse; pairs
    with a -1 (an ended walk) are dropped.  ORDER: offset-major, then position, then walk, then (forward, reverse) -- a reference can
    equal it entry for entry.  Plain slicing, no kernel; repeated pairs and (v, v) stay (EdgeSet.from_walks collapses them)."""
    L = int(walks.shape[1]) - 1
    src, dst = [], []
    for o in range(1, min(int(window), L) + 1):
        a, b = walks[:, :L + 1 - o].t().reshape(-1), walks[:, o:].t().reshape(-1)      # position-major, then walk
        keep = (a >= 0) & (b >= 0)
        a, b = a[keep], b[keep]
        src.append(torch.stack([a, b], 1).reshape(-1))
        dst.append(torch.stack([b, a], 1).reshape(-1))
    if not src:
        e = torch.empty(0, dtype=torch.int32, device=walks.device)
        return e, e.clone()
    return torch.cat(src).to(torch.int32), torch.cat(dst).to(torch.int32)


class ReceptiveField:
    """The L-hop receptive field of a query set on a CsrGraph, built once and reusable (a validation mask evaluated every epoch).
    With Q_L = the query's rows and Q_{l-1} = the columns stored in rows Q_l of CSR(A) (no self term: the diagonal is not stored):
      rows[l]   l = 0..L   ascending int32 rows of the graph (row order, nid applied); a row's compact id is its position
      nnz[l]    l = 1..L   entries of the block of A with rows Q_l and columns Q_{l-1} (nnz[0] is 0)
      block[l]  l = 1..L   (rowptr, colidx) of that block, entries in stored order, columns as positions in rows[l - 1]
      norm[l]   l = 1..L   g.norm on rows[l];   plan[l]: an SpmmPlan of the block when the graph has plans (same arguments)
      n_query, query_rows (the query's rows in the caller's order), query_pos (their compact rows in rows[L])
    Needs g.norm; the transposed CSR is not used."""

    def __init__(self, g, query, n_layers):
        if g.norm is None:
            raise ValueError("receptive_field() needs the norm (from_coo(norm=True))")
        L = int(n_layers)
        if L < 1:
            raise ValueError("n_layers must be at least 1")
        q = query.reshape(-1)
        if q.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or query.dim() != 1:
            raise ValueError("query must be a 1-D integer tensor of vertex ids")
        dev = g.rowptr.device
        q = q.to(dev).long()
        self.n_query = int(q.numel())
        if self.n_query and (int(q.min()) < 0 or int(q.max()) >= g.n):
            raise ValueError(f"query holds a vertex id outside [0, {g.n})")
        r = q if g.nid is None else g.nid[q].long()
        self.g, self.n, self.n_layers = g, g.n, L
        member = torch.zeros(g.n, dtype=torch.uint8, device=dev)
        member[r] = 1
        self.rows = [None] * (L + 1)
        self.rows[L] = rows_from_mask(member)
        self.query_rows = r.to(torch.int32)
        self.query_pos = rows_to_positions(self.rows[L], g.n)[r].contiguous()
        self.nnz, self.block, self.norm, self.plan = [0] * (L + 1), [None] * (L + 1), [None] * (L + 1), [None] * (L + 1)
        for l in range(L, 0, -1):
            k = int(self.rows[l].numel())
            self.rows[l - 1], self.nnz[l] = _frontier(g.rowptr, g.colidx, self.rows[l], g.n)
            pos = rows_to_positions(self.rows[l - 1], g.n)
            rp, ci, _ = csr_extract_rows(g.rowptr, g.colidx, self.rows[l], col_pos=pos, n_cols=g.n, nnz_capacity=self.nnz[l])
            self.block[l] = (rp, ci)
            self.norm[l] = gather_rows(g.norm.reshape(-1, 1), self.rows[l]).reshape(-1) if k else g.norm[:0]
            if g.plan is not None and k:
                chunk, max_feat, big_rows = g._plan_args
                self.plan[l] = SpmmPlan(rp, chunk, max_feat)
                if big_rows is not None:
                    self.plan[l].set_big_row_threshold(big_rows)
        self.compact_rows = torch.arange(int(self.rows[L].numel()), dtype=torch.int32, device=dev)


def _inv_deg(rowptr):
    """1 / (entries of a row), 0 for an empty row: the division on the host -- IEEE, rounded once."""
    deg = (rowptr[1:] - rowptr[:-1]).cpu().to(torch.float32)
    return torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg)).to(rowptr.device)


class SampledField:
    """The sampled L-layer field of a batch of seed vertices on a CsrGraph -- what one mini-batch GraphSAGE step reads
    (SageStack.predict / batch_step), at a cost of O(batch * product of the fanouts) plus one O(n) mark and one O(n) position table per
    layer.  L = len(fanouts); layer l (1 .. L) keeps at most fanouts[l - 1] stored neighbours per row, drawn by sample_rows from the
    layer's seed.  With Q_L = the seeds' rows and Q_{l-1} = Q_l united with the columns kept for rows Q_l (a layer reads the vertex
    itself through W_s, so Q_l is a subset of Q_{l-1}):
      rows[l]      l = 0..L   ascending int32 rows of the graph (row order, nid applied); a row's compact id is its position
      nnz[l]       l = 1..L   kept entries of the block with rows Q_l (nnz[0] is 0)
      block[l]     l = 1..L   (rowptr, colidx): row x is row rows[l][x] of g.sample_neighbors(fanouts[l - 1], seeds[l - 1]), entries in
                              stored order, columns as positions in rows[l - 1]
      self_pos[l]  l = 1..L   int32 [|Q_l|], the position of rows[l][x] in rows[l - 1]
      inv_deg[l]   l = 1..L   1 / (entries of block row x), 0 for an empty one
      block_t[l]   l = 1..L   (rowptr_t, colidx_t) of the transposed block, |Q_{l-1}| rows, built from the COO (column, list position)
      map_t(l)                csr_transpose_map of block l, built on first use (aggr="max"); GnnxError on a relabelled graph
      seeds                   the L layer seeds; n_query, query_rows (the seeds' rows in the caller's order), query_pos (their compact
                              rows in rows[L])
    seed: an int s gives layer l the seed s * L + (l - 1), so seed=epoch never reuses a layer seed across epochs; or a sequence of L
    ints.  seeds: a 1-D integer tensor of VERTEX ids, any order; a repeated id counts once in rows[L].  No plans are built: a block row
    has at most 64 entries."""

    def __init__(self, g, seeds, fanouts, seed):
        fan = [int(k) for k in fanouts]
        L = len(fan)
        if L < 1:
            raise ValueError("fanouts must name at least one layer")
        if isinstance(seed, (list, tuple)):
            if len(seed) != L:
                raise ValueError(f"{len(seed)} seeds for {L} layers")
            self.seeds = [int(s) for s in seed]
        else:
            self.seeds = [int(seed) * L + l for l in range(L)]
        q = seeds.reshape(-1)
        if q.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or seeds.dim() != 1:
            raise ValueError("seeds must be a 1-D integer tensor of vertex ids")
        dev = g.rowptr.device
        q = q.to(dev).long()
        self.n_query = int(q.numel())
        if self.n_query and (int(q.min()) < 0 or int(q.max()) >= g.n):
            raise ValueError(f"seeds hold a vertex id outside [0, {g.n})")
        r = q if g.nid is None else g.nid[q].long()
        self.g, self.n, self.n_layers, self.fanouts = g, g.n, L, fan
        member = torch.zeros(g.n, dtype=torch.uint8, device=dev)
        member[r] = 1
        self.rows = [None] * (L + 1)
        self.rows[L] = rows_from_mask(member)
        self.query_rows = r.to(torch.int32)
        self.query_pos = rows_to_positions(self.rows[L], g.n)[r].contiguous()
        self.nnz, self.block, self.block_t = [0] * (L + 1), [None] * (L + 1), [None] * (L + 1)
        self.self_pos, self.inv_deg, self._map_t = [None] * (L + 1), [None] * (L + 1), [None] * (L + 1)
        mark = member   # rows[L] are marked already
        for l in range(L, 0, -1):
            rows_l = self.rows[l]
            rp, ci, _, rowid = sample_rows(g.rowptr, g.colidx, rows_l, fan[l - 1], self.seeds[l - 1], n_cols=g.n, want_rowid=True, col_mark=mark)
            self.rows[l - 1] = rows_from_mask(mark)
            pos = rows_to_positions(self.rows[l - 1], g.n)
            renumber_cols(ci, pos)
            m_in, e = int(self.rows[l - 1].numel()), int(ci.numel())
            self.nnz[l], self.block[l] = e, (rp, ci)
            self.self_pos[l] = pos[rows_l.long()].contiguous()
            self.inv_deg[l] = _inv_deg(rp)
            if e:   # the square builder suffices: |Q_l| <= |Q_{l-1}|; self loops and duplicates kept -- exactly the kept entries
                self.block_t[l] = CsrGraph.csr_from_coo(ci, rowid, m_in, flags=3)
            else:
                self.block_t[l] = (torch.zeros(m_in + 1, dtype=torch.int32, device=dev), ci)
            # (the marks stay: the next layer's rows are marked already, as Q_{l-1} contains Q_l)
        self.compact_rows = torch.arange(int(self.rows[L].numel()), dtype=torch.int32, device=dev)

    def map_t(self, l):
        """csr_transpose_map of block l (built once): spmm_reduce's arg reaches the transposed block through it."""
        if self.g.nid is not None:
            raise capi.GnnxError(-7, "SampledField.map_t", "a relabelled graph keeps each row in original-id order, not ascending: the "
                                 "transpose map cannot be built on it (build the graph without relabel)")
        if self._map_t[l] is None:
            (rp, ci), (rpt, cit) = self.block[l], self.block_t[l]
            # (a rectangular pattern: |Q_l| rows against the |Q_{l-1}| rows of its transpose; no entries: nothing to map)
            self._map_t[l] = csr_transpose_map(rp, ci, rpt, cit) if self.nnz[l] else ci
        return self._map_t[l]


def to_bf16(X, out=None):
    """f32 -> bf16 feature storage (torch.bfloat16 tensor, same shape) for spmm(..., X bf16)."""
    out = torch.empty(X.shape, dtype=torch.bfloat16, device=X.device) if out is None else out
    capi.call("gnnx_f32_to_bf16", _ptr(X), _ld(X), X.shape[0], X.shape[1], _ptr(out), _ld(out), _stream())
    return out


def linear_fwd_bf16(X, W, out=None):
    """OPT-IN (bf16 feature storage): H = X . W^T as a torch.bfloat16 tensor.  gnnx_gemm_nt_bf16out_f32 (the product's epilogue
    rounds and stores bf16) on the LDS-DMA kernel's shapes, else the product followed by to_bf16: the same bits either way."""
    M, K = X.shape
    N = W.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=X.device) if out is None else out
    ok = (K % 64 == 0 and N % 4 == 0 and N >= 64 and M >= 2048 and _ld(X) % 4 == 0 and _ld(out) % 4 == 0 and X.data_ptr() % 16 == 0
          and out.data_ptr() % 16 == 0)
    if not ok:
        return to_bf16(gemm(X, W, transB=True), out=out)
    ws, wsb = _scratch("gnnx_gemm_nt_bf16out_workspace", M, N, K, device=X.device, tag="gemm_bf16out")
    capi.call("gnnx_gemm_nt_bf16out_f32", M, N, K, _ptr(X), _ld(X), _ptr(W), _ld(W), _ptr(out), _ld(out), _ptr(ws), wsb, _stream())
    return out


DIAG_KEEP, DIAG_STRIP, DIAG_FILL = 0, 1, 2
CSR_KEEP_DUPLICATES, CSR_DROP_TRUNCATED_ZERO = 2, 4


def csr_from_coo_weighted(src, dst, w, n_nodes, diag_mode=DIAG_KEEP, diag_value=0.0, flags=0):
    """Weighted adjacency A[r][c] = w, last duplicate wins (edge_attr, reference graph.cpp:21-75) -> (rowptr, colidx, vals)."""
    E = int(src.numel())
    dev = src.device
    cap = max(E + n_nodes, 1)
    rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    colidx = torch.empty(cap, dtype=torch.int32, device=dev)
    vals = torch.empty(cap, dtype=torch.float32, device=dev)
    wsb = C.c_size_t(0)
    capi.call("gnnx_csr_from_coo_weighted_workspace", E, n_nodes, C.byref(wsb))
    ws = torch.empty(max(wsb.value, 1), dtype=torch.uint8, device=dev)
    nnz = C.c_int64(0)
    capi.call("gnnx_csr_from_coo_weighted", _ptr(src), _ptr(dst), _ptr(w), E, n_nodes, int(flags), int(diag_mode), float(diag_value),
              _ptr(rowptr), _ptr(colidx), _ptr(vals), C.byref(nnz), _ptr(ws), ws.numel(), _stream())
    return rowptr, colidx[: nnz.value].clone(), vals[: nnz.value].clone()


def csr_rowsum(rowptr, vals=None, out=None):
    n = int(rowptr.numel() - 1)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=rowptr.device)
    assert out.numel() == n and out.is_contiguous()
    capi.call("gnnx_csr_rowsum_f32", _ptr(rowptr), _ptr(vals), n, _ptr(out), _stream())
    return out


def spmm(rowptr, colidx, X, out=None, vals=None, colscale=None, rowscale=None, bias=None, beta=0.0, plan=None,
         n_rows=None, bn=None, relu_in=False, relu_out=False):
    """gnnx_spmm_csr_f32: Y = beta*Y + rowscale (.) (A . (colscale (.) X)) + bias.
    bn=(mean, var, gamma|None, beta|None, eps) / relu_in / relu_out: gnnx_spmm_csr_fused_f32 (BatchNorm / ReLU applied to
    every gathered row, ReLU on the stored row)."""
    n_rows = int(rowptr.numel() - 1) if n_rows is None else n_rows
    n_cols, F = X.shape
    if out is None:
        out = torch.empty((n_rows, F), dtype=torch.float32, device=X.device)
    if X.dtype == torch.bfloat16:  # opt-in bf16 feature storage: half the gather bytes, f32 accumulation
        capi.call("gnnx_spmm_csr_bf16_f32", n_rows, n_cols, F, _ptr(rowptr), _ptr(colidx), _ptr(vals), _ptr(colscale),
                  _ptr(rowscale), _ptr(bias), _ptr(X), _ld(X), float(beta), _ptr(out), _ld(out),
                  plan.h if plan is not None else None, _stream())
        return out
    if bn is not None or relu_in or relu_out:
        mean, var, gamma, bbeta, eps = bn if bn is not None else (None, None, None, None, 0.0)
        addr = lambda t: None if t is None else _ptr(t).value  # noqa: E731
        fu = capi.SpmmFusion(addr(mean), addr(var), addr(gamma), addr(bbeta), float(eps), int(relu_in), int(relu_out))
        capi.call("gnnx_spmm_csr_fused_f32", n_rows, n_cols, F, _ptr(rowptr), _ptr(colidx), _ptr(vals), _ptr(colscale),
                  _ptr(rowscale), _ptr(bias), _ptr(X), _ld(X), float(beta), _ptr(out), _ld(out), C.byref(fu),
                  plan.h if plan is not None else None, _stream())
        return out
    capi.call("gnnx_spmm_csr_f32", n_rows, n_cols, F, _ptr(rowptr), _ptr(colidx), _ptr(vals), _ptr(colscale),
              _ptr(rowscale), _ptr(bias), _ptr(X), _ld(X), float(beta), _ptr(out), _ld(out),
              plan.h if plan is not None else None, _stream())
    return out


def sddmm(rowptr, colidx, L, R, rowscale=None, colscale=None, out=None):
    """gnnx_sddmm_csr_f32: out[p] = (<L[i,:], R[c_p,:]> * rowscale[i]) * colscale[c_p] for every stored entry p of row i -- float32
    [nnz].  L: [n_rows, F], R: [n_cols, F] (L is R is allowed).  The dot product's order is a function of F alone (include/gnnx.h)."""
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    n_cols, F = R.shape
    if L.shape[0] != n_rows or L.shape[1] != F:
        raise capi.GnnxError(-2, "sddmm", f"L is {tuple(L.shape)}, the pattern has {n_rows} rows and R {F} features")
    if out is None:
        out = torch.empty(nnz, dtype=torch.float32, device=R.device)
    assert out.numel() == nnz and out.is_contiguous()
    capi.call("gnnx_sddmm_csr_f32", n_rows, n_cols, F, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(L) if L.numel() else None, _ld(L),
              _ptr(R) if R.numel() else None, _ld(R), _ptr(rowscale), _ptr(colscale), _ptr(out) if nnz else None, _stream())
    return out


def spmm_vals_grad(rowptr, colidx, G, X, rowscale=None, colscale=None):
    """dL/dvals of Y = rowscale (.) sum_p vals[p] * colscale[c_p] * X[c_p,:] (spmm) for the upstream gradient G = dL/dY: the dense
    G . X^T of the reference's MatMul::_backward (operation.h:516-523) on the stored entries only -- sddmm(L = G, R = X)."""
    return sddmm(rowptr, colidx, G, X, rowscale=rowscale, colscale=colscale)


def csr_transpose_map(rowptr, colidx, rowptr_t, colidx_t):
    """gnnx_csr_transpose_map: int32 [nnz], map_t[q] = the position in CSR(A) of entry q of CSR(A^T); vals[map_t.long()] (or
    gather_rows on a [nnz, 1] view) carries per-entry values to the transposed order.  GnnxError (status -3) when the two are not
    each other's transpose with strictly ascending rows."""
    n_rows, n_cols, nnz = int(rowptr.numel() - 1), int(rowptr_t.numel() - 1), int(colidx.numel())
    if int(colidx_t.numel()) != nnz:
        raise capi.GnnxError(-3, "csr_transpose_map", f"{nnz} entries against {int(colidx_t.numel())} in the transposed pattern")
    map_t = torch.empty(nnz, dtype=torch.int32, device=rowptr.device)
    capi.call("gnnx_csr_transpose_map", n_rows, n_cols, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(rowptr_t),
              _ptr(colidx_t) if nnz else None, _ptr(map_t) if nnz else None, _stream())
    return map_t


def bce_logits(scores, target, want_grad=True, n_total=None, grad_out=None):
    """gnnx_bce_logits_f32: (mean binary cross-entropy of the logits `scores` against the float targets -- soft labels allowed -- as a
    1-element device tensor, dscores = (sigmoid(scores) - target) / n_total or None).  n_total: the divisor (default: len(scores))."""
    n = int(scores.numel())
    assert scores.is_contiguous() and target.is_contiguous() and target.dtype == torch.float32 and int(target.numel()) == n
    loss = torch.empty(1, dtype=torch.float32, device=scores.device)
    d = (torch.empty_like(scores) if grad_out is None else grad_out) if want_grad else None
    assert d is None or (d.is_contiguous() and d.numel() == n)
    ws, wsb = _scratch("gnnx_bce_logits_workspace", n, device=scores.device, tag="bce")
    capi.call("gnnx_bce_logits_f32", _ptr(scores) if n else None, _ptr(target) if n else None, n, int(n if n_total is None else n_total),
              _ptr(loss), _ptr(d), _ptr(ws), wsb, _stream())
    return loss, d


class EdgeSet:
    """Labelled vertex pairs as a sparse pattern: the CSR of the pairs (rowptr, colidx) with the per-entry targets `target`, the
    transposed pattern (rowptr_t, colidx_t) and map_t (csr_transpose_map) -- what a stack's link_scores / link_train_step score, and what
    sends the score gradient back to both endpoints without atomics."""

    def __init__(self, n, rowptr, colidx, target, rowptr_t, colidx_t, map_t):
        self.n = int(n)
        self.rowptr, self.colidx, self.target = rowptr, colidx, target
        self.rowptr_t, self.colidx_t, self.map_t = rowptr_t, colidx_t, map_t
        self.nnz = int(colidx.numel())

    @classmethod
    def from_pairs(cls, src, dst, label, n):
        """src, dst: int32 endpoints in the graph's ROW order (g.nid[v] of vertex ids on a relabelled graph); label: float32 per pair
        (1 = an edge, 0 = a non-edge; soft labels allowed); n: the number of vertices.  The pattern is built with
        csr_from_coo_weighted(src, dst, label, DIAG_KEEP): of duplicate pairs the LAST one in the list wins, and explicit 0 labels stay
        as entries.  So negatives concatenated BEFORE the positives lose a collision with a positive: a sampled "non-edge" that is in
        fact an edge is scored as the edge it is.  Uniform negatives: rmat_edges(seed, n, k, a=.25, b=.25, c=.25); negatives drawn from
        the non-edges of a graph: from_graph."""
        src, dst = src.to(torch.int32).contiguous(), dst.to(torch.int32).contiguous()
        label = label.to(torch.float32).contiguous()
        rowptr, colidx, target = csr_from_coo_weighted(src, dst, label, n, DIAG_KEEP)
        rowptr_t, colidx_t, _ = csr_from_coo_weighted(dst, src, label, n, DIAG_KEEP)
        return cls(n, rowptr, colidx, target, rowptr_t, colidx_t, csr_transpose_map(rowptr, colidx, rowptr_t, colidx_t))

    @classmethod
    def from_graph(cls, g, m, seed, positives=None):
        """The positives (an EdgeSet or a (rowptr, colidx) pair on g's rows; default: every stored entry of g) with target 1 and m
        negatives per positive with target 0, drawn by g.sample_negatives(m, seed, positives): the destination of each positive
        replaced by a column its row does not hold in g, never the row itself.  Built through from_pairs with the negatives listed
        BEFORE the positives, as its docstring prescribes; a negative is never an edge of g, so it can only collide with another
        negative: repeated draws of one row collapse into one entry there, and unfilled draws (rows that hold every column) are
        dropped -- the pattern holds at most nnz_pos * (1 + m) entries.  link_train_step(X, EdgeSet.from_graph(g, 1, seed=epoch), lr)
        is an epoch with fresh negatives."""
        rowptr, colidx = (g.rowptr, g.colidx) if positives is None else _pattern_of(positives, "from_graph")
        neg, _ = g.sample_negatives(m, seed, (rowptr, colidx))
        deg = (rowptr[1:] - rowptr[:-1]).long()
        rows = torch.repeat_interleave(torch.arange(g.n, dtype=torch.int32, device=rowptr.device), deg)
        nsrc, ndst = torch.repeat_interleave(rows, int(m)), neg.reshape(-1)
        keep = ndst >= 0
        nsrc, ndst = nsrc[keep], ndst[keep]
        label = torch.cat([torch.zeros(nsrc.numel(), dtype=torch.float32, device=rows.device),
                           torch.ones(rows.numel(), dtype=torch.float32, device=rows.device)])
        return cls.from_pairs(torch.cat([nsrc, rows]), torch.cat([ndst, colidx.to(torch.int32)]), label, g.n)

    @classmethod
    def from_walks(cls, g, walks, window, m, seed):
        """The co-occurrence pairs of random walks on g as positives, m negatives per positive off g: the unsupervised objective of
        DeepWalk / node2vec and of GraphSAGE section 3.2.  The positives pattern is walk_pairs(walks, window) through
        CsrGraph.csr_from_coo with its default flags -- repeated pairs collapse into one entry, (v, v) is dropped, rows are ascending --
        and the result is from_graph(g, m, seed, positives=pattern): a negative is never an edge of g nor the row itself, but may be a
        walk partner that is not an edge, and loses a collision with a positive as from_pairs prescribes.
        net.link_train_step(X, EdgeSet.from_walks(g, g.random_walk(batch, 5, seed=ep), 2, 1, seed=ep), lr) is one unsupervised epoch."""
        src, dst = walk_pairs(walks, window)
        return cls.from_graph(g, m, seed, positives=CsrGraph.csr_from_coo(src, dst, g.n))

    def to_transposed(self, vals, out=None):
        """Per-entry values of the pattern in the transposed pattern's order: out[q] = vals[map_t[q]]."""
        if out is None:
            out = torch.empty(self.nnz, dtype=torch.float32, device=vals.device)
        if self.nnz:
            gather_rows(vals.reshape(-1, 1), self.map_t, out=out.reshape(-1, 1))
        return out


EDGE_SOFTMAX_UNNORMALISED = 1


def _edge_term(t, n, what):
    """(pointer, stride in elements) of a per-vertex term: float32 [n], contiguous or a 1-D strided view (a column of an [n, 2] matrix)."""
    if t is None:
        return None, 0
    if t.dim() != 1 or int(t.numel()) != n or t.dtype != torch.float32:
        raise capi.GnnxError(-2, "edge_softmax", f"{what} must be a float32 vector of {n} entries, got {tuple(t.shape)} {t.dtype}")
    stride = int(t.stride(0)) if n > 1 else 1
    if stride < 1:
        raise capi.GnnxError(-1, "edge_softmax", f"{what} has stride {stride}")
    return _ptr(t), stride


def _edge_softmax_args(rowptr, colidx, scores, rowterm, colterm):
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    if scores is not None and (int(scores.numel()) != nnz or not scores.is_contiguous() or scores.dtype != torch.float32):
        raise capi.GnnxError(-2, "edge_softmax", f"scores must be a contiguous float32 vector of {nnz} entries")
    n_cols = int(colterm.numel()) if colterm is not None else n_rows
    rt, rs = _edge_term(rowterm, n_rows, "rowterm")
    ct, cs = _edge_term(colterm, n_cols, "colterm")
    ws, _ = _scratch("gnnx_edge_softmax_workspace", n_rows, nnz, device=rowptr.device, tag="edge_softmax")
    return n_rows, n_cols, nnz, rt, rs, ct, cs, ws


def edge_softmax(rowptr, colidx, scores=None, rowterm=None, colterm=None, negative_slope=1.0, unnormalised=False, want_stats=False):
    """gnnx_edge_softmax_csr_f32: alpha[p] = softmax over the stored entries of row i of leaky_relu((scores[p] + rowterm[i]) +
    colterm[c_p]) -- float32 [nnz]; operands that are None are skipped (at least one is needed), slope 1 is the identity.  rowterm /
    colterm: float32 [n_rows] / [n_cols], 1-D strided views allowed (the two columns of an [n, 2] matrix).  unnormalised: exp(e_p - max_i)
    instead.  want_stats: (alpha, rowmax, rowsum).  The order of the row sums is a function of the row length alone (include/gnnx.h)."""
    n_rows, n_cols, nnz, rt, rs, ct, cs, ws = _edge_softmax_args(rowptr, colidx, scores, rowterm, colterm)
    dev = rowptr.device
    out = torch.empty(nnz, dtype=torch.float32, device=dev)
    rowmax = torch.empty(n_rows, dtype=torch.float32, device=dev) if want_stats else None
    rowsum = torch.empty(n_rows, dtype=torch.float32, device=dev) if want_stats else None
    capi.call("gnnx_edge_softmax_csr_f32", n_rows, n_cols, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(scores), rt, rs, ct, cs,
              float(negative_slope), EDGE_SOFTMAX_UNNORMALISED if unnormalised else 0, _ptr(out) if nnz else None, _ptr(rowmax), _ptr(rowsum),
              _ptr(ws), ws.numel(), _stream())
    return (out, rowmax, rowsum) if want_stats else out


def edge_softmax_bwd(rowptr, colidx, alpha, dalpha, scores=None, rowterm=None, colterm=None, negative_slope=1.0, drowterm_out=None):
    """gnnx_edge_softmax_bwd_csr_f32: (dt, drowterm) from alpha = edge_softmax(...) of the same operands and dalpha = dL/dalpha.  dt
    [nnz] is the gradient of scores; drowterm [n_rows] (the row sums of dt) that of rowterm; the gradient of colterm is
    csr_rowsum(rowptr_t, dt[map_t]) on the transposed pattern (CsrGraph.attention_map / csr_transpose_map)."""
    n_rows, n_cols, nnz, rt, rs, ct, cs, ws = _edge_softmax_args(rowptr, colidx, scores, rowterm, colterm)
    for t, what in ((alpha, "alpha"), (dalpha, "dalpha")):
        if int(t.numel()) != nnz or not t.is_contiguous() or t.dtype != torch.float32:
            raise capi.GnnxError(-2, "edge_softmax_bwd", f"{what} must be a contiguous float32 vector of {nnz} entries")
    dev = rowptr.device
    dt = torch.empty(nnz, dtype=torch.float32, device=dev)
    drow = torch.empty(n_rows, dtype=torch.float32, device=dev) if drowterm_out is None else drowterm_out
    assert drow.numel() == n_rows and drow.is_contiguous()
    capi.call("gnnx_edge_softmax_bwd_csr_f32", n_rows, n_cols, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(scores), rt, rs, ct, cs,
              float(negative_slope), _ptr(alpha) if nnz else None, _ptr(dalpha) if nnz else None, _ptr(dt) if nnz else None, _ptr(drow),
              _ptr(ws), ws.numel(), _stream())
    return dt, drow


def _entry_major(t, nnz, H, what, where):
    """Leading dimension of a per-entry, per-head array: float32 [nnz, H], unit stride along the heads (a column slab of a wider
    [nnz, ld] array is fine)."""
    if t.dim() != 2 or tuple(t.shape) != (nnz, H) or t.dtype != torch.float32 or (H > 1 and t.stride(1) != 1):
        raise capi.GnnxError(-2, where, f"{what} must be an entry-major float32 [{nnz}, {H}] array, got {tuple(t.shape)} {t.dtype}")
    return int(t.stride(0)) if nnz > 1 else H


def _heads_of(X, n_heads, where):
    F = int(X.shape[1])
    if n_heads < 1 or F % n_heads or F == 0:
        raise capi.GnnxError(-2, where, f"{F} features do not split into {n_heads} heads")
    return F // n_heads


def csr_rowsum_heads(rowptr, vals, out=None):
    """gnnx_csr_rowsum_heads_f32: out[i, h] = the sum of vals[p, h] over the entries p of row i, added in ascending p from +0 -- column h
    carries the bits of csr_rowsum(rowptr, vals[:, h]).  vals: entry-major float32 [nnz, H]; out: [n_rows, H], a column slab of a wider
    matrix allowed."""
    n_rows, nnz, H = int(rowptr.numel() - 1), int(vals.shape[0]), int(vals.shape[1])
    ldv = _entry_major(vals, nnz, H, "vals", "csr_rowsum_heads")
    if out is None:
        out = torch.empty((n_rows, H), dtype=torch.float32, device=rowptr.device)
    op, ldo = _edge_terms_heads(out, n_rows, H, "out")
    capi.call("gnnx_csr_rowsum_heads_f32", _ptr(rowptr), _ptr(vals) if nnz else None, ldv, n_rows, H, op, ldo, _stream())
    return out


def spmm_heads(rowptr, colidx, X, vals, n_heads, bias=None, beta=0.0, relu_out=False, out=None):
    """gnnx_spmm_csr_heads_f32: Y[i, hD + j] = beta*Y + sum_p vals[p, h] * X[c_p, hD + j] + bias, optional ReLU -- head h carries the bits
    of spmm(vals = vals[:, h]) on column slab h of X.  X: [n_cols, H*D]; vals: entry-major float32 [nnz, H] (a slab of a wider array is
    fine); out: [n_rows, H*D], a column slab of a wider matrix allowed (the other columns are not touched).  No plan: a row is one lane
    group's chain."""
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    n_cols = int(X.shape[0])
    D = _heads_of(X, n_heads, "spmm_heads")
    ldv = _entry_major(vals, nnz, n_heads, "vals", "spmm_heads")
    if out is None:
        out = torch.empty((n_rows, n_heads * D), dtype=torch.float32, device=X.device)
    assert tuple(out.shape) == (n_rows, n_heads * D) and (bias is None or int(bias.numel()) == n_heads * D)
    # an empty pattern has no entry to read: any non-null pointer stands in for the two per-entry arrays
    capi.call("gnnx_spmm_csr_heads_f32", n_rows, n_cols, n_heads, D, _ptr(rowptr), _ptr(colidx) if nnz else _ptr(rowptr),
              _ptr(vals) if nnz else _ptr(rowptr), ldv, _ptr(bias), _ptr(X), _ld(X), float(beta), int(bool(relu_out)), _ptr(out), _ld(out), _stream())
    return out


def sddmm_heads(rowptr, colidx, L, R, n_heads, out=None):
    """gnnx_sddmm_csr_heads_f32: out[p, h] = <L[i, slab h], R[c_p, slab h]> for every stored entry p of row i -- entry-major float32
    [nnz, H]; head h carries the bits of sddmm on column slab h.  L: [n_rows, H*D], R: [n_cols, H*D] (L is R is allowed)."""
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    n_cols = int(R.shape[0])
    D = _heads_of(R, n_heads, "sddmm_heads")
    if tuple(L.shape) != (n_rows, n_heads * D):
        raise capi.GnnxError(-2, "sddmm_heads", f"L is {tuple(L.shape)}, the pattern has {n_rows} rows and R {n_heads * D} features")
    if out is None:
        out = torch.empty((nnz, n_heads), dtype=torch.float32, device=R.device)
    ldo = _entry_major(out, nnz, n_heads, "out", "sddmm_heads")
    capi.call("gnnx_sddmm_csr_heads_f32", n_rows, n_cols, n_heads, D, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(L), _ld(L),
              _ptr(R), _ld(R), _ptr(out) if nnz else None, ldo, _stream())
    return out


def _gatv2_vector(a, F, where):
    if a.dim() != 1 or int(a.numel()) != F or a.dtype != torch.float32 or not a.is_contiguous():
        raise capi.GnnxError(-2, where, f"a must be a contiguous float32 [{F}] vector, got {tuple(a.shape)} {a.dtype}")


def gatv2_scores(rowptr, colidx, L, R, a, n_heads, negative_slope=0.2, out=None):
    """gnnx_gatv2_scores_csr_f32: out[p, h] = sum_k a[hD + k] * leaky_relu(L[i, hD + k] + R[c_p, hD + k]) for every stored entry p of row
    i -- the GATv2 score, entry-major float32 [nnz, H], summed in the lane-group order of sddmm_heads.  L: [n_rows, H*D], R: [n_cols, H*D]
    (column slabs of wider matrices are fine; L is R is allowed); a: float32 [H*D], head h's vector in its slab."""
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    n_cols = int(R.shape[0])
    D = _heads_of(R, n_heads, "gatv2_scores")
    if tuple(L.shape) != (n_rows, n_heads * D):
        raise capi.GnnxError(-2, "gatv2_scores", f"L is {tuple(L.shape)}, the pattern has {n_rows} rows and R {n_heads * D} features")
    _gatv2_vector(a, n_heads * D, "gatv2_scores")
    if out is None:
        out = torch.empty((nnz, n_heads), dtype=torch.float32, device=R.device)
    ldo = _entry_major(out, nnz, n_heads, "out", "gatv2_scores")
    capi.call("gnnx_gatv2_scores_csr_f32", n_rows, n_cols, n_heads, D, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, _ptr(L), _ld(L),
              _ptr(R), _ld(R), _ptr(a), float(negative_slope), _ptr(out) if nnz else None, ldo, _stream())
    return out


def gatv2_scores_bwd(rowptr, colidx, de, own, other, a, n_heads, negative_slope=0.2, entry_map=None, out=None, beta=0.0, want_T=False,
                     T_out=None):
    """gnnx_gatv2_scores_bwd_csr_f32: the gradient of gatv2_scores to the ROW-SIDE operand of the pattern it is handed,
        out[i, f] = beta*out + sum_p de[m_p, h] * (u > 0 ? a[f] : a[f] * slope),  u = own[i, f] + other[c_p, f],  m_p = entry_map[p] or p,
    one accumulator per element over the row's entries from the last down (spmm_heads' order).  On the forward pattern (own = L, other = R)
    it is dL; on the transposed pattern with entry_map = the transpose map (de stays in the forward order) and beta = 1 it adds dR onto
    `out`.  want_T: also T[i, f] = sum_p de[m_p, h] * leaky_relu(u), whose colsum is the gradient of a; returns (out, T) then, else out.
    de: entry-major float32 [nnz, H]; own: [n_rows, H*D]; other: [n_cols, H*D]; out / T_out: [n_rows, H*D], column slabs allowed."""
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    n_cols = int(other.shape[0])
    D = _heads_of(other, n_heads, "gatv2_scores_bwd")
    F = n_heads * D
    if tuple(own.shape) != (n_rows, F):
        raise capi.GnnxError(-2, "gatv2_scores_bwd", f"own is {tuple(own.shape)}, the pattern has {n_rows} rows and other {F} features")
    _gatv2_vector(a, F, "gatv2_scores_bwd")
    ldd = _entry_major(de, nnz, n_heads, "de", "gatv2_scores_bwd")
    if entry_map is not None and (entry_map.dtype != torch.int32 or int(entry_map.numel()) != nnz or not entry_map.is_contiguous()):
        raise capi.GnnxError(-2, "gatv2_scores_bwd", f"entry_map must be a contiguous int32 [{nnz}] array")
    if out is None:
        if beta:
            raise capi.GnnxError(-2, "gatv2_scores_bwd", "beta = 1 adds onto `out`, which was not given")
        out = torch.empty((n_rows, F), dtype=torch.float32, device=own.device)
    T = T_out
    if want_T and T is None:
        T = torch.empty((n_rows, F), dtype=torch.float32, device=own.device)
    assert tuple(out.shape) == (n_rows, F) and (T is None or tuple(T.shape) == (n_rows, F))
    capi.call("gnnx_gatv2_scores_bwd_csr_f32", n_rows, n_cols, n_heads, D, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None,
              _ptr(de) if nnz else None, ldd, _ptr(entry_map) if nnz else None, _ptr(own), _ld(own), _ptr(other), _ld(other), _ptr(a),
              float(negative_slope), float(beta), _ptr(out), _ld(out), _ptr(T), _ld(T) if T is not None else F, _stream())
    return (out, T) if T is not None else out


def _edge_terms_heads(t, n, H, what):
    """(pointer, row stride in elements) of a per-vertex, per-head term: float32 [n, H] with unit stride along the heads (one half of an
    [n, 2H] matrix is fine)."""
    if t is None:
        return None, 0
    if t.dim() != 2 or tuple(t.shape) != (n, H) or t.dtype != torch.float32 or (H > 1 and t.stride(1) != 1):
        raise capi.GnnxError(-2, "edge_softmax_heads", f"{what} must be a float32 [{n}, {H}] array, got {tuple(t.shape)} {t.dtype}")
    return _ptr(t), (int(t.stride(0)) if n > 1 else H)


def _edge_softmax_heads_args(rowptr, colidx, n_heads, scores, rowterm, colterm):
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    lds = _entry_major(scores, nnz, n_heads, "scores", "edge_softmax_heads") if scores is not None else n_heads
    n_cols = int(colterm.shape[0]) if colterm is not None else n_rows
    rt, rs = _edge_terms_heads(rowterm, n_rows, n_heads, "rowterm")
    ct, cs = _edge_terms_heads(colterm, n_cols, n_heads, "colterm")
    ws, _ = _scratch("gnnx_edge_softmax_heads_workspace", n_rows, nnz, n_heads, device=rowptr.device, tag="edge_softmax")
    return n_rows, n_cols, nnz, lds, rt, rs, ct, cs, ws


def edge_softmax_heads(rowptr, colidx, n_heads, scores=None, rowterm=None, colterm=None, negative_slope=1.0, unnormalised=False,
                       want_stats=False, out=None):
    """gnnx_edge_softmax_csr_heads_f32: edge_softmax per head -- alpha entry-major float32 [nnz, H]; scores [nnz, H], rowterm [n_rows, H],
    colterm [n_cols, H] (each optional; the two halves of one [n, 2H] matrix serve as the terms).  want_stats: (alpha, rowmax, rowsum)
    with the statistics as [n_rows, H].  Head h carries the bits of edge_softmax on column h of every operand."""
    n_rows, n_cols, nnz, lds, rt, rs, ct, cs, ws = _edge_softmax_heads_args(rowptr, colidx, n_heads, scores, rowterm, colterm)
    dev = rowptr.device
    if out is None:
        out = torch.empty((nnz, n_heads), dtype=torch.float32, device=dev)
    ldo = _entry_major(out, nnz, n_heads, "out", "edge_softmax_heads")
    rowmax = torch.empty((n_rows, n_heads), dtype=torch.float32, device=dev) if want_stats else None
    rowsum = torch.empty((n_rows, n_heads), dtype=torch.float32, device=dev) if want_stats else None
    capi.call("gnnx_edge_softmax_csr_heads_f32", n_rows, n_cols, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, n_heads,
              _ptr(scores) if nnz else None, lds, rt, rs, ct, cs, float(negative_slope), EDGE_SOFTMAX_UNNORMALISED if unnormalised else 0,
              _ptr(out) if nnz else None, ldo, _ptr(rowmax), _ptr(rowsum), _ptr(ws), ws.numel(), _stream())
    return (out, rowmax, rowsum) if want_stats else out


def edge_softmax_heads_bwd(rowptr, colidx, n_heads, alpha, dalpha, scores=None, rowterm=None, colterm=None, negative_slope=1.0,
                           drowterm_out=None, dt_out=None):
    """gnnx_edge_softmax_bwd_csr_heads_f32: (dt [nnz, H], drowterm [n_rows, H]) from alpha = edge_softmax_heads(...) of the same operands
    and dalpha = dL/dalpha, all entry-major.  drowterm_out: a float32 [n_rows, H] view with unit stride along the heads, e.g. the left
    half of an [n, 2H] buffer."""
    n_rows, n_cols, nnz, lds, rt, rs, ct, cs, ws = _edge_softmax_heads_args(rowptr, colidx, n_heads, scores, rowterm, colterm)
    lda = _entry_major(alpha, nnz, n_heads, "alpha", "edge_softmax_heads_bwd")
    ldd = _entry_major(dalpha, nnz, n_heads, "dalpha", "edge_softmax_heads_bwd")
    dev = rowptr.device
    dt = torch.empty((nnz, n_heads), dtype=torch.float32, device=dev) if dt_out is None else dt_out
    ldt = _entry_major(dt, nnz, n_heads, "dt", "edge_softmax_heads_bwd")
    drow = torch.empty((n_rows, n_heads), dtype=torch.float32, device=dev) if drowterm_out is None else drowterm_out
    dp, drs = _edge_terms_heads(drow, n_rows, n_heads, "drowterm_out")
    capi.call("gnnx_edge_softmax_bwd_csr_heads_f32", n_rows, n_cols, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None, n_heads,
              _ptr(scores) if nnz else None, lds, rt, rs, ct, cs, float(negative_slope), _ptr(alpha) if nnz else None, lda,
              _ptr(dalpha) if nnz else None, ldd, _ptr(dt) if nnz else None, ldt, dp, drs, _ptr(ws), ws.numel(), _stream())
    return dt, drow


REDUCE_OPS = {"max": 0, "min": 1}   # GNNX_REDUCE_MAX / GNNX_REDUCE_MIN


def spmm_reduce(rowptr, colidx, X, op="max", vals=None, out=None, arg_out=None, want_arg=True):
    """gnnx_spmm_csr_reduce_f32: (Y, arg) with Y[i, f] = max (op="min": min) over the stored entries p of row i of vals[p] * X[c_p, f]
    (X[c_p, f] itself without vals) and arg[i, f] = the first position p that attains it -- int32, absolute in colidx; an empty row
    gives +0 and -1.  want_arg=False: arg is None and not computed.  The bits are a function of the inputs alone (include/gnnx.h
    "neighbourhood reductions")."""
    if op not in REDUCE_OPS:
        raise capi.GnnxError(-1, "spmm_reduce", f"op must be 'max' or 'min', got {op!r}")
    n_rows, nnz = int(rowptr.numel() - 1), int(colidx.numel())
    n_cols, F = X.shape
    if vals is not None and (int(vals.numel()) != nnz or not vals.is_contiguous() or vals.dtype != torch.float32):
        raise capi.GnnxError(-2, "spmm_reduce", f"vals must be a contiguous float32 vector of {nnz} entries")
    if out is None:
        out = torch.empty((n_rows, F), dtype=torch.float32, device=X.device)
    arg = (torch.empty((n_rows, F), dtype=torch.int32, device=X.device) if arg_out is None else arg_out) if want_arg else None
    assert tuple(out.shape) == (n_rows, F) and (arg is None or (tuple(arg.shape) == (n_rows, F) and arg.dtype == torch.int32))
    ws, _ = _scratch("gnnx_spmm_csr_reduce_workspace", n_rows, nnz, F, device=X.device, tag="reduce")
    capi.call("gnnx_spmm_csr_reduce_f32", REDUCE_OPS[op], n_rows, n_cols, F, nnz, _ptr(rowptr), _ptr(colidx) if nnz else None,
              _ptr(vals) if nnz else None, _ptr(X) if X.numel() else None, _ld(X), _ptr(out), _ld(out), _ptr(arg),
              _ld(arg) if arg is not None else 0, _ptr(ws), ws.numel(), _stream())
    return out, arg


def spmm_reduce_bwd(rowptr_t, colidx_t, map_t, arg, G, vals=None, out=None, beta=0.0):
    """gnnx_spmm_csr_reduce_bwd_f32: dX = beta * dX + the gradient of spmm_reduce with respect to X, on the TRANSPOSED pattern: entry q
    of row c of CSR(A^T) adds vals[map_t[q]] * G[i, f] (i = colidx_t[q]) where arg[i, f] == map_t[q].  map_t: csr_transpose_map; vals in
    the order of CSR(A).  No atomics: a documented order (include/gnnx.h), the same bits every run."""
    n_rows_t, nnz = int(rowptr_t.numel() - 1), int(colidx_t.numel())
    n_cols_t, F = G.shape
    if tuple(arg.shape) != (n_cols_t, F) or arg.dtype != torch.int32 or int(map_t.numel()) != nnz:
        raise capi.GnnxError(-2, "spmm_reduce_bwd", f"arg must be int32 {(n_cols_t, F)} and map_t have {nnz} entries")
    if vals is not None and (int(vals.numel()) != nnz or not vals.is_contiguous() or vals.dtype != torch.float32):
        raise capi.GnnxError(-2, "spmm_reduce_bwd", f"vals must be a contiguous float32 vector of {nnz} entries")
    if out is None:
        if beta != 0.0:
            raise capi.GnnxError(-1, "spmm_reduce_bwd", "beta = 1 needs the matrix to add to (out)")
        out = torch.empty((n_rows_t, F), dtype=torch.float32, device=G.device)
    assert tuple(out.shape) == (n_rows_t, F)
    ws, _ = _scratch("gnnx_spmm_csr_reduce_workspace", n_rows_t, nnz, F, device=G.device, tag="reduce")
    capi.call("gnnx_spmm_csr_reduce_bwd_f32", n_rows_t, n_cols_t, F, nnz, _ptr(rowptr_t), _ptr(colidx_t) if nnz else None,
              _ptr(map_t) if nnz else None, _ptr(vals) if nnz else None, _ptr(arg) if arg.numel() else None, _ld(arg),
              _ptr(G) if G.numel() else None, _ld(G), float(beta), _ptr(out), _ld(out), _ptr(ws), ws.numel(), _stream())
    return out


def transpose(X, out=None):
    """gnnx_transpose_f32: out[c, r] = X[r, c] (materialised)."""
    R, Cn = X.shape
    if out is None:
        out = torch.empty((Cn, R), dtype=torch.float32, device=X.device)
    capi.call("gnnx_transpose_f32", _ptr(X), _ld(X), R, Cn, _ptr(out), _ld(out), _stream())
    return out


def gemm(A, B, transA=False, transB=False, out=None, alpha=1.0, beta=0.0):
    """gnnx_gemm_f32: C = alpha * op(A) . op(B) + beta * C (row-major, no operand is transposed in memory)."""
    M = A.shape[1] if transA else A.shape[0]
    K = A.shape[0] if transA else A.shape[1]
    N = B.shape[0] if transB else B.shape[1]
    Kb = B.shape[1] if transB else B.shape[0]
    if K != Kb:
        raise capi.GnnxError(-2, "gemm", f"inner dimensions differ: {K} vs {Kb}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    wsb = capi.gemm_workspace(transA, transB, M, N, K)
    ws = _workspace(wsb, A.device, "gemm") if wsb else None
    capi.call("gnnx_gemm_f32", int(transA), int(transB), M, N, K, float(alpha), _ptr(A), _ld(A), _ptr(B), _ld(B),
              float(beta), _ptr(out), _ld(out), _ptr(ws), wsb, _stream())
    return out


def gemm_relu_colsum(A, B, Ymask, out=None, colsum_out=None):
    """gnnx_gemm_relu_colsum_f32: C = (A . B) (.) (Ymask > 0), colsum = column sums of C -- the stacked layers' backward step
    G_{l-1} = (dH_l . W_l) (.) relu'(Y_{l-1}), db_{l-1} = colsum(G_{l-1}) in one pass over the output."""
    M, K = A.shape
    N = B.shape[1]
    out = torch.empty((M, N), dtype=torch.float32, device=A.device) if out is None else out
    colsum_out = torch.empty(N, dtype=torch.float32, device=A.device) if colsum_out is None else colsum_out
    ws, wsb = _scratch("gnnx_gemm_relu_colsum_workspace", M, N, K, device=A.device, tag="gemm_fuse")
    capi.call("gnnx_gemm_relu_colsum_f32", M, N, K, _ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(Ymask), _ld(Ymask), _ptr(out), _ld(out),
              _ptr(colsum_out), _ptr(ws), wsb, _stream())
    return out, colsum_out


def linear_fwd_bn_stats(X, W, out=None):
    """OPT-IN gnnx_gemm_bn_stats_f32: H = X . W^T and the BatchNorm batch statistics of H in one pass (single-pass shifted
    variance: within rounding of bn_stats(H), not bit-equal).  Returns (H, mean, var)."""
    M, K = X.shape
    N = W.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=X.device) if out is None else out
    mean = torch.empty(N, dtype=torch.float32, device=X.device)
    var = torch.empty(N, dtype=torch.float32, device=X.device)
    ws, wsb = _scratch("gnnx_gemm_bn_stats_workspace", M, N, K, device=X.device, tag="gemm_bn")
    capi.call("gnnx_gemm_bn_stats_f32", M, N, K, _ptr(X), _ld(X), _ptr(W), _ld(W), _ptr(out), _ld(out), _ptr(mean), _ptr(var), _ptr(ws),
              wsb, _stream())
    return out, mean, var


def gemm_split(A, B, transB=False, out=None):
    """OPT-IN split-precision GEMM (gnnx_gemm_split_bf16_f32): A[M,K] . op(B) on the bf16 matrix cores from exact 3-way bf16
    splits of the f32 operands, f32 accumulation; f32-level accuracy, not the reference's arithmetic."""
    M, K = A.shape
    N = B.shape[0] if transB else B.shape[1]
    out = torch.empty((M, N), dtype=torch.float32, device=A.device) if out is None else out
    ws, wsb = _scratch("gnnx_gemm_split_workspace", M, N, K, device=A.device, tag="gemm_split")
    capi.call("gnnx_gemm_split_bf16_f32", int(transB), M, N, K, _ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(out), _ld(out), _ptr(ws),
              wsb, _stream())
    return out


def colsum(G, out=None, beta=0.0):
    N, F = G.shape
    if out is None:
        out = torch.empty(F, dtype=torch.float32, device=G.device)
    wsb = capi.colsum_workspace(N, F)
    ws = _workspace(wsb, G.device, "colsum")
    capi.call("gnnx_colsum_f32", _ptr(G), _ld(G), N, F, float(beta), _ptr(out), _ptr(ws), wsb, _stream())
    return out


SLOTS_PER_ROW = 8   # gnnx_rows_to_slots_f32: a row goes to at most world - 1 <= 7 peers


def slot_table(send_idx, n_rows):
    """[n_rows, 8] int32 for rows_to_slots: row r's positions in the send buffer (send_idx[slot] == r), ascending, packed to the
    front, -1 behind.  None when some row has more than 7 slots (more than 7 peers read it: use the gather pack)."""
    dev = send_idx.device
    table = torch.full((max(int(n_rows), 1), SLOTS_PER_ROW), -1, dtype=torch.int32, device=dev)
    if int(send_idx.numel()) == 0:
        return table
    order = torch.sort(send_idx.to(torch.int64), stable=True).indices        # slots grouped by row, ascending slot inside a row
    rows = send_idx.to(torch.int64)[order]
    first = torch.searchsorted(rows, rows, right=False)
    k = torch.arange(rows.numel(), device=dev) - first                          # rank of the slot among its row's slots
    if int(k.max()) >= SLOTS_PER_ROW - 1:
        return None
    table[rows, k] = order.to(torch.int32)
    return table


def rows_to_slots(X, table, send, colsum_out=None, beta=0.0):
    """gnnx_rows_to_slots_f32: the halo pack from the producer's side -- every row of X read once and written to each of its send
    slots (table = slot_table(send_idx, n_rows)); colsum_out: the column sums of all rows of X from the same pass (the bits of
    colsum())."""
    N, F = X.shape
    ws, wsb = None, 0
    if colsum_out is not None:
        wsb = capi.colsum_workspace(N, F)
        ws = _workspace(wsb, X.device, "colsum")
    capi.call("gnnx_rows_to_slots_f32", _ptr(X), _ld(X), N, F, _ptr(table), _ptr(send), _ld(send), _ptr(colsum_out) if colsum_out is not None else None,
              float(beta), _ptr(ws) if ws is not None else None, wsb, _stream())
    return send


def linear_fwd_rows_to_slots(X, W, out, table, send):
    """gnnx_gemm_nt_rows_to_slots_f32: H = X . W^T (linear_fwd's bits) with the halo pack in the product's epilogue -- every row of H
    listed in `table` (slot_table) also stored to its rows of `send`, from the registers H is stored from (rows_to_slots' bytes without
    the pass that reads H back)."""
    M, K = X.shape
    N = W.shape[0]
    ws, wsb = _scratch("gnnx_gemm_nt_rows_to_slots_workspace", M, N, K, device=X.device, tag="gemm")
    capi.call("gnnx_gemm_nt_rows_to_slots_f32", M, N, K, _ptr(X), _ld(X), _ptr(W), _ld(W), _ptr(out), _ld(out), _ptr(table), _ptr(send), _ld(send),
              _ptr(ws), wsb, _stream())
    return out


def gather_row_stride(n_rows, n_feat):
    """gnnx_gather_row_stride: the row pitch (floats) for a matrix whose rows the aggregation gathers (n_feat, or n_feat + 64 for large
    matrices of 512-byte-multiple rows: spreads the hub rows of a synthetic power-law graph over the memory channels)."""
    ld = C.c_int64(0)
    capi.call("gnnx_gather_row_stride", int(n_rows), int(n_feat), C.byref(ld))
    return ld.value


def empty_gathered(n_rows, n_feat, device="cuda"):
    """An uninitialised [n_rows, n_feat] view of a buffer on the gather pitch (gather_row_stride)."""
    ld = gather_row_stride(n_rows, n_feat)
    return torch.empty((n_rows, ld), dtype=torch.float32, device=device)[:, :n_feat]


def colsum_copy(G, copy, out=None, beta=0.0):
    """gnnx_colsum_copy_f32: column sums of G (as colsum, same bits) and, from the same pass, G's rows copied into `copy` (a view on
    another row stride: empty_gathered)."""
    N, F = G.shape
    if out is None:
        out = torch.empty(F, dtype=torch.float32, device=G.device)
    wsb = capi.colsum_workspace(N, F)
    ws = _workspace(wsb, G.device, "colsum")
    capi.call("gnnx_colsum_copy_f32", _ptr(G), _ld(G), N, F, float(beta), _ptr(out), _ptr(copy), _ld(copy), _ptr(ws), wsb, _stream())
    return out


def gather_rows(X, idx, out=None):
    n, F = int(idx.numel()), X.shape[1]
    if out is None:
        out = torch.empty((n, F), dtype=torch.float32, device=X.device)
    capi.call("gnnx_gather_rows_f32", _ptr(X), _ld(X), _ptr(idx), n, F, _ptr(out), _ld(out), _stream())
    return out


def scatter_add_rows(inp, idx, Y):
    n, F = int(idx.numel()), inp.shape[1]
    capi.call("gnnx_scatter_add_rows_f32", _ptr(inp), _ld(inp), _ptr(idx), n, F, _ptr(Y), _ld(Y), _stream())
    return Y


def rowscale(X, v, out=None):
    out = torch.empty_like(X) if out is None else out
    capi.call("gnnx_rowscale_f32", _ptr(X), _ld(X), _ptr(v), X.shape[0], X.shape[1], _ptr(out), _ld(out), _stream())
    return out


def bias_add(X, b, out=None):
    out = torch.empty_like(X) if out is None else out
    capi.call("gnnx_bias_add_f32", _ptr(X), _ld(X), _ptr(b), X.shape[0], X.shape[1], _ptr(out), _ld(out), _stream())
    return out


_BINARY_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3}


def binary(op, A, B, out=None):
    """`A (op) B` with the API's 2-D broadcast (reference functional.h:163-239, utils.h:181-228): each operand is [N,F],
    [N,1], [1,F], [F] or a one-element tensor."""
    def as2d(t):
        return t.reshape(1, -1) if t.dim() <= 1 else t
    A2, B2 = as2d(A), as2d(B)
    n, f = max(A2.shape[0], B2.shape[0]), max(A2.shape[1], B2.shape[1])
    for t in (A2, B2):
        if t.shape[0] not in (1, n) or t.shape[1] not in (1, f) or not t.is_contiguous():
            raise ValueError("operands are not broadcastable 2-D contiguous tensors")
    strides = lambda t: (t.shape[1] if t.shape[0] == n and n > 1 else 0, 1 if t.shape[1] == f and f > 1 else 0)  # noqa: E731
    out = torch.empty((n, f), dtype=torch.float32, device=A.device) if out is None else out
    (ars, acs), (brs, bcs) = strides(A2), strides(B2)
    capi.call("gnnx_binary_bcast_f32", _BINARY_OPS[op], n, f, _ptr(A2), ars, acs, _ptr(B2), brs, bcs, _ptr(out), _ld(out), _stream())
    return out


def rowsum(X, out=None):
    out = torch.empty((X.shape[0],), dtype=torch.float32, device=X.device) if out is None else out
    capi.call("gnnx_rowsum_f32", _ptr(X), _ld(X), X.shape[0], X.shape[1], _ptr(out), _stream())
    return out


def axpy(a, x, y):
    capi.call("gnnx_axpy_f32", x.numel(), float(a), _ptr(x), _ptr(y), _stream())
    return y


def bn_stats(X):
    """Batch mean / biased variance per feature (x->mean(-2), x->var(-2, 0); reference nn.cpp:303,312)."""
    N, F = X.shape
    mean = torch.empty(F, dtype=torch.float32, device=X.device)
    var = torch.empty(F, dtype=torch.float32, device=X.device)
    ws, wsb = _scratch("gnnx_bn_workspace", N, F, device=X.device, tag="bn")
    capi.call("gnnx_bn_stats_f32", _ptr(X), _ld(X), N, F, _ptr(mean), _ptr(var), _ptr(ws), wsb, _stream())
    return mean, var


def bn_partial(X, mean=None, scale=1.0):
    """scale * column sums of X (mean None) or of (X - mean)^2: the per-shard halves of the batch statistics (gnnx_bn_partial_f32)."""
    N, F = X.shape
    out = torch.empty(F, dtype=torch.float32, device=X.device)
    ws, wsb = _scratch("gnnx_bn_workspace", N, F, device=X.device, tag="bn")
    capi.call("gnnx_bn_partial_f32", _ptr(X), _ld(X), N, F, _ptr(mean), float(scale), _ptr(out), _ptr(ws), wsb, _stream())
    return out


def bn_relu_fwd(X, mean=None, var=None, gamma=None, beta=None, eps=1e-5, relu=True, out=None):
    out = torch.empty_like(X) if out is None else out
    capi.call("gnnx_bn_relu_fwd_f32", _ptr(X), _ld(X), X.shape[0], X.shape[1], _ptr(mean), _ptr(var), float(eps), _ptr(gamma),
              _ptr(beta), int(relu), _ptr(out), _ld(out), _stream())
    return out


def bn_relu_bwd(X, Y, dY, mean=None, var=None, gamma=None, eps=1e-5, relu=True, beta=None, reference_quirk=False, out=None):
    """Y=None with relu: the forward output was never stored (fused forward); its sign is recomputed from X.
    reference_quirk: gnnx_bn_relu_bwd_quirk_f32, the gradient the REFERENCE's traversal delivers (statistics as constants)."""
    N, F = X.shape
    dX = torch.empty_like(X) if out is None else out
    dgamma = torch.empty(F, dtype=torch.float32, device=X.device) if mean is not None else None
    dbeta = torch.empty(F, dtype=torch.float32, device=X.device) if mean is not None else None
    ws, wsb = _scratch("gnnx_bn_workspace", N, F, device=X.device, tag="bn")
    capi.call("gnnx_bn_relu_bwd_quirk_f32" if reference_quirk else "gnnx_bn_relu_bwd_f32", _ptr(X), _ld(X), _ptr(Y),
              _ld(Y) if Y is not None else 0, _ptr(dY), _ld(dY), N, F, _ptr(mean),
              _ptr(var), float(eps), _ptr(gamma), _ptr(beta), int(relu), _ptr(dX), _ld(dX), _ptr(dgamma), _ptr(dbeta), _ptr(ws),
              wsb, _stream())
    return dX, dgamma, dbeta


def bn_relu_bwd_sums(X, Y, dY, mean, var, gamma=None, eps=1e-5, relu=True, beta=None):
    """gnnx_bn_relu_bwd_sums_f32: (dgamma, dbeta) over THIS call's rows -- the first half of bn_relu_bwd, which a sharded BatchNorm
    all-reduces before the apply half."""
    N, F = X.shape
    dgamma = torch.empty(F, dtype=torch.float32, device=X.device)
    dbeta = torch.empty(F, dtype=torch.float32, device=X.device)
    ws, wsb = _scratch("gnnx_bn_workspace", N, F, device=X.device, tag="bn")
    capi.call("gnnx_bn_relu_bwd_sums_f32", _ptr(X), _ld(X), _ptr(Y), _ld(Y) if Y is not None else 0, _ptr(dY), _ld(dY), N, F, _ptr(mean),
              _ptr(var), float(eps), _ptr(gamma), _ptr(beta), int(relu), _ptr(dgamma), _ptr(dbeta), _ptr(ws), wsb, _stream())
    return dgamma, dbeta


def bn_relu_bwd_apply(X, Y, dY, mean=None, var=None, gamma=None, dgamma=None, dbeta=None, n_total=None, eps=1e-5, relu=True, beta=None,
                      out=None):
    """gnnx_bn_relu_bwd_apply_f32: dX of this call's rows from the (global) sums and the (global) row count n_total."""
    N, F = X.shape
    dX = torch.empty((N, F), dtype=torch.float32, device=X.device) if out is None else out
    ws, wsb = _scratch("gnnx_bn_workspace", N, F, device=X.device, tag="bn")
    capi.call("gnnx_bn_relu_bwd_apply_f32", _ptr(X), _ld(X), _ptr(Y), _ld(Y) if Y is not None else 0, _ptr(dY), _ld(dY), N, F, _ptr(mean),
              _ptr(var), float(eps), _ptr(gamma), _ptr(beta), int(relu), _ptr(dgamma), _ptr(dbeta), int(N if n_total is None else n_total),
              _ptr(dX), _ld(dX), _ptr(ws), wsb, _stream())
    return dX


def fill(x, value):
    """gnnx_fill_f32 on a contiguous tensor."""
    assert x.is_contiguous()
    capi.call("gnnx_fill_f32", _ptr(x), x.numel(), float(value), _stream())
    return x


def rmat_edges(seed, n_nodes, n_edges, a=0.57, b=0.19, c=0.19, device="cuda", first_edge=0):
    src = torch.empty(n_edges, dtype=torch.int32, device=device)
    dst = torch.empty(n_edges, dtype=torch.int32, device=device)
    capi.call("gnnx_rmat_edges", int(seed), int(n_nodes), int(n_edges), int(first_edge), float(a), float(b), float(c),
              _ptr(src), _ptr(dst), _stream())
    return src, dst


def uniform_pm1(seed, shape, scale=1.0, device="cuda"):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    capi.call("gnnx_uniform_pm1_f32", int(seed), out.numel(), float(scale), _ptr(out), _stream())
    return out


# ---- the hot path, chained as the reference chains it ------------------------------------------------
def linear_fwd(X, W, out=None):
    """H = X . W^T  (nn.cpp:205-211; GCNConv's lin has no bias, graph.cpp:162)."""
    return gemm(X, W, transB=True, out=out)


def aggregate_fwd(g, H, bias=None, out=None, use_plan=True, bn=None, relu_in=False, relu_out=False, labelled=None):
    """out = norm (.) (A . H) (+ bias)  (graph.cpp:204-212, :188).  bn / relu_in: GCNConv's BatchNorm + ReLU between transform
    and aggregation (graph.cpp:174-175) folded into the gather; relu_out: the ReLU in front of the next layer.
    labelled (CsrGraph.labelled): the same call on the row-restricted CSR -- labelled rows have the full aggregation's bits, every
    other row holds `bias` (not computed)."""
    c = g if labelled is None else labelled
    return spmm(c.rowptr, c.colidx, H, out=out, rowscale=g.norm, bias=bias, plan=c.plan if use_plan else None, bn=bn,
                relu_in=relu_in, relu_out=relu_out)


def aggregate_bwd(g, G, out=None, beta=0.0, use_plan=True, labelled=None):
    """dH = A^T . (norm (.) G)  (operation.h:144-167 then :524-531).
    The per-source scale norm[i] is handed to the kernel per non-zero (vals_t[p] = norm[colidx_t[p]], gathered once per
    graph): a coalesced 4 B/edge stream instead of a random 4-byte gather per edge; the arithmetic (one rounded multiply
    per term) is identical.
    labelled (CsrGraph.labelled): G is zero outside the labelled rows; the same call on the column-restricted CSR(A^T) -- the
    dropped terms are norm * 0, the result has the full product's bits."""
    if labelled is not None:
        return spmm(labelled.rowptr_t, labelled.colidx_t, G, out=out, vals=labelled.norm_per_nz_t, beta=beta,
                    plan=labelled.plan_t if use_plan else None)
    if getattr(g, "norm_per_nz_t", None) is None:
        g.norm_per_nz_t = gather_rows(g.norm.reshape(-1, 1), g.colidx_t).reshape(-1)
    return spmm(g.rowptr_t, g.colidx_t, G, out=out, vals=g.norm_per_nz_t, beta=beta, plan=g.plan_t if use_plan else None)


def aggregate_bwd_bn_sums(g, G, H, mean, var, gamma=None, beta=None, eps=1e-5, relu=True, out=None, use_plan=True):
    """gnnx_spmm_csr_bn_sums_f32: dY = A^T . (norm (.) G) as aggregate_bwd computes it (same bits) plus BatchNorm's backward column
    sums dgamma / dbeta over g = dY masked by relu(BN(H)) -- accumulated by the wavefronts that store dY, so the separate sums
    pass over dY and H disappears.  Returns (dY, dgamma, dbeta); follow with gnnx_bn_relu_bwd_apply_f32."""
    if getattr(g, "norm_per_nz_t", None) is None:
        g.norm_per_nz_t = gather_rows(g.norm.reshape(-1, 1), g.colidx_t).reshape(-1)
    n, F = G.shape
    if out is None:
        out = torch.empty((n, F), dtype=torch.float32, device=G.device)
    dgamma = torch.empty(F, dtype=torch.float32, device=G.device)
    dbeta = torch.empty(F, dtype=torch.float32, device=G.device)
    plan = g.plan_t if use_plan else None
    ph = plan.h if plan is not None else None
    ws, wsb = _scratch("gnnx_spmm_csr_bn_sums_workspace", n, F, ph, device=G.device, tag="bn_sums")
    capi.call("gnnx_spmm_csr_bn_sums_f32", n, n, F, _ptr(g.rowptr_t), _ptr(g.colidx_t), _ptr(g.norm_per_nz_t), _ptr(G), _ld(G), _ptr(out),
              _ld(out), _ptr(H), _ld(H), _ptr(mean), _ptr(var), float(eps), _ptr(gamma), _ptr(beta), int(relu), _ptr(dgamma), _ptr(dbeta),
              _ptr(ws), wsb, ph, _stream())
    return out, dgamma, dbeta


def aggregate_fwd_sym(g, H, bias=None, out=None, self_term=False, use_plan=True):
    """Mode SYM, the textbook layer the north_star writes: out = D^-1/2 A D^-1/2 . H (+ bias), s = (1 + deg)^-1/2 as in the
    reference's degree block (graph.cpp:178,183); with self_term the D^-1/2 (A + I) D^-1/2 form.  Unlike Mode REF (the
    reference's factorised norm, graph.cpp:196-199) the scale is applied per edge: colscale = s, rowscale = s."""
    out = spmm(g.rowptr, g.colidx, H, out=out, colscale=g.s, rowscale=g.s, bias=bias, plan=g.plan if use_plan else None)
    if self_term:  # + s_i^2 * H_i
        s2 = g.s * g.s
        axpy(1.0, rowscale(H, s2), out)
    return out


def aggregate_bwd_sym(g, G, out=None, self_term=False, use_plan=True):
    """dH = D^-1/2 A^T D^-1/2 . G (+ s^2 (.) G): the same kernel on the transposed CSR."""
    out = spmm(g.rowptr_t, g.colidx_t, G, out=out, colscale=g.s, rowscale=g.s, plan=g.plan_t if use_plan else None)
    if self_term:
        axpy(1.0, rowscale(G, g.s * g.s), out)
    return out


def linear_bwd(dH, X, W, dX=None, dW=None, beta_dw=0.0):
    """dX = dH . W ; dW = dH^T . X  (operation.h:516-531, :416-433)."""
    dX = gemm(dH, W, out=dX)
    dW = gemm(dH, X, transA=True, out=dW, beta=beta_dw)
    return dX, dW


def gcn_layer_fwd(g, X, W, bias):
    H = linear_fwd(X, W)
    out = aggregate_fwd(g, H, bias)
    return H, out


def gcn_layer_bwd(g, X, W, G):
    dbias = colsum(G)
    dH = aggregate_bwd(g, G)
    dX, dW = linear_bwd(dH, X, W)
    return dict(dbias=dbias, dH=dH, dX=dX, dW=dW)


# ---- whole training step: multi-layer GCN + softmax cross-entropy + SGD ----------
def _softmax_ce(logits, target, rows, d, colsum_out, n_total):
    """The one call behind softmax_ce (rows is None: every row) and softmax_ce_rows; d: the gradient buffer or None."""
    N, Cn = logits.shape
    n = N if rows is None else int(rows.numel())
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    assert colsum_out is None or (d is not None and colsum_out.numel() == Cn and colsum_out.is_contiguous())
    if rows is not None:
        query = ("gnnx_softmax_ce_rows_workspace", n, Cn)
    elif colsum_out is not None:
        query = ("gnnx_softmax_ce_colsum_workspace", n, Cn)
    else:
        query = ("gnnx_softmax_ce_workspace", n)
    ws, _ = _scratch(*query, device=logits.device, tag="ce")
    tail = (int(n if n_total is None else n_total), _ptr(loss), _ptr(d), 0 if d is None else _ld(d), _ptr(colsum_out), _ptr(ws), ws.numel(),
            _stream())
    if rows is None:
        capi.call("gnnx_softmax_ce_partial_f32", _ptr(logits), _ld(logits), _ptr(target), N, Cn, *tail)
    else:
        capi.call("gnnx_softmax_ce_rows_f32", _ptr(logits), _ld(logits), _ptr(target), _ptr(rows) if n else None, n, N, Cn, *tail)
    return loss, d


def softmax_ce(logits, target, want_grad=True, colsum_out=None, n_total=None, grad_out=None):
    """(mean loss as a 1-element device tensor, dlogits or None): gnnx_softmax_ce_f32 (reference forward nn.cpp:442-453).
    colsum_out [C]: also the column sums of dlogits (the last layer's bias gradient), from the kernel that writes dlogits.
    n_total: the rows are one shard of a batch of n_total (gnnx_softmax_ce_partial_f32: loss = this rank's term of the mean).
    grad_out: where dlogits goes (e.g. the [:n_local] rows of a [local | halo] buffer)."""
    d = (torch.empty_like(logits) if grad_out is None else grad_out) if want_grad else None
    return _softmax_ce(logits, target, None, d, colsum_out, n_total)


def softmax_ce_rows(logits, target, rows, colsum_out=None, grad_out=None, n_total=None, want_grad=True):
    """gnnx_softmax_ce_rows_f32: (loss over the listed rows / n_total as a 1-element device tensor, dlogits or None).  Only the listed
    rows of the gradient buffer are written: pass a zeroed grad_out (without one a zero-filled buffer is made).  target is read at
    listed rows only.  colsum_out [C]: the column sums of the listed gradient rows.  n_total: the divisor (default: len(rows))."""
    d = (torch.zeros_like(logits) if grad_out is None else grad_out) if want_grad else None
    return _softmax_ce(logits, target, rows, d, colsum_out, n_total)


def argmax_rows(logits):
    """gnnx_argmax_rows_f32: int32 [N], the first index of each row's maximum (reference functional.h:59-61)."""
    N, Cn = logits.shape
    pred = torch.empty(max(N, 1), dtype=torch.int32, device=logits.device)
    ws = _workspace(512, logits.device, "argmax")
    capi.call("gnnx_argmax_rows_f32", _ptr(logits), _ld(logits), N, Cn, _ptr(pred), _ptr(ws), ws.numel(), _stream())
    return pred[:N]


def accuracy(logits, target, rows=None):
    """gnnx_accuracy_rows_f32: (number of listed rows -- all rows without a list -- whose argmax equals the target, number of rows
    counted) as Python ints."""
    N, Cn = logits.shape
    nl = N if rows is None else int(rows.numel())
    ws = _workspace(512, logits.device, "argmax")
    correct = C.c_int64(0)
    capi.call("gnnx_accuracy_rows_f32", _ptr(logits), _ld(logits), _ptr(target), _ptr(rows) if (rows is not None and nl) else None, nl, N, Cn,
              None, C.byref(correct), _ptr(ws), ws.numel(), _stream())
    return correct.value, nl


def _loss_and_accuracy(logits, target, rows):
    """(loss over `rows` as a 1-element tensor, correct predictions among them, len(rows)) of a forward's logits."""
    return (softmax_ce_rows(logits, target, rows, want_grad=False)[0], *accuracy(logits, target, rows))


def sgd_step(param, grad, lr, weight_decay=0.0):
    capi.call("gnnx_sgd_step_f32", _ptr(param), _ptr(grad), param.numel(), float(lr), float(weight_decay), _stream())
    return param


class _TableOptimizer:
    """What Adam and Momentum share: the parameter table of gnnx_optim_table_build over a model's params() / grads(), built at the
    first step together with zeroed state arenas (`n_state` of them), the step count `t`, and gradient clipping by the global norm
    (max_grad_norm: gnnx_grad_sqnorm_f32 writes the scale on the device; the update reads it there).  A step is one launch -- two with
    clipping -- however many tensors the model has.  The table holds addresses: a step on parameter or gradient tensors other than
    the bound ones raises; it never rebuilds (the state would silently start over)."""

    n_state = 1

    def __init__(self, max_grad_norm=None):
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError(f"max_grad_norm must be >= 0, got {max_grad_norm!r}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.t = 0
        self._bound = None

    def _bind(self, params, grads):
        n = len(params)
        for p, g in zip(params, grads):
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not (p.is_contiguous() and g.is_contiguous()) or p.numel() != g.numel():
                raise ValueError("the optimiser needs contiguous float32 parameters with gradients of the same size")
        dev = params[0].device
        self._sizes = [p.numel() for p in params]
        self._bound = [p.data_ptr() for p in params] + [g.data_ptr() for g in grads]
        nbytes, chunks, elems = C.c_size_t(0), C.c_int64(0), C.c_int64(0)
        capi.call("gnnx_optim_table_bytes", n, C.byref(nbytes))
        self._table = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        capi.call("gnnx_optim_table_build", n, (C.c_void_p * n)(*self._bound[:n]), (C.c_void_p * n)(*self._bound[n:]),
                  (C.c_int64 * n)(*self._sizes), _ptr(self._table), nbytes.value, C.byref(chunks), C.byref(elems), _stream())
        self._n, self._chunks = n, chunks.value
        self._arenas = [torch.zeros(max(elems.value, 1), dtype=torch.float32, device=dev) for _ in range(self.n_state)]
        self._offsets = [sum((s + 3) // 4 * 4 for s in self._sizes[:k]) for k in range(n)]
        ws = C.c_size_t(0)
        capi.call("gnnx_grad_sqnorm_workspace", C.byref(ws))
        self._norm_ws = torch.empty(ws.value, dtype=torch.uint8, device=dev)
        self.sqnorm = torch.zeros(1, dtype=torch.float32, device=dev)    # of the last clipped step's gradients
        self.gscale = torch.ones(1, dtype=torch.float32, device=dev)     # and the factor they were multiplied with

    def step(self, params, grads, lr, weight_decay=0.0):
        """One update of `params` from `grads` (the model's lists; _Model.step calls this)."""
        if self._bound is None:
            self._bind(params, grads)
        now = [p.data_ptr() for p in params] + [g.data_ptr() for g in grads]
        if now != self._bound:
            k = next((i for i, (a, b) in enumerate(zip(now, self._bound)) if a != b), min(len(now), len(self._bound)))
            raise RuntimeError(f"the optimiser is bound to {self._n} tensors at fixed addresses; "
                               + (f"this step has {len(params)} tensors" if len(now) != len(self._bound) else
                                  f"{'parameter' if k < self._n else 'gradient'} {k % self._n} has moved from {self._bound[k]:#x} to {now[k]:#x}")
                               + " (one optimiser per model; its state is not rebuilt)")
        scale = None
        if self.max_grad_norm is not None:
            capi.call("gnnx_grad_sqnorm_f32", _ptr(self._table), self._n, self.max_grad_norm, _ptr(self.sqnorm), _ptr(self.gscale),
                      _ptr(self._norm_ws), self._norm_ws.numel(), _stream())
            scale = self.gscale
        self._update(float(lr), float(weight_decay), _ptr(scale))
        self.t += 1

    def _views(self, arena):
        return [arena[o:o + s] for o, s in zip(self._offsets, self._sizes)]


class Adam(_TableOptimizer):
    """Adam (Kingma & Ba 2015); decoupled=True: AdamW (Loshchilov & Hutter 2019).  The arithmetic is include/gnnx.h's, one float32
    rounding per operation; the betas are rounded to float32 once, here; the bias corrections 1 - beta^t come from
    gnnx_adam_bias_corrections.  net.set_optimizer(ops.Adam()) -- lr and weight_decay stay arguments of step / train_step."""

    n_state = 2

    def __init__(self, betas=(0.9, 0.999), eps=1e-8, decoupled=False, max_grad_norm=None):
        super().__init__(max_grad_norm)
        self.b1, self.b2 = (C.c_float(b).value for b in betas)
        if not (0.0 <= self.b1 < 1.0 and 0.0 <= self.b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {betas!r}")
        if not eps > 0:
            raise ValueError(f"eps must be > 0, got {eps!r}")
        self.eps, self.decoupled = float(eps), bool(decoupled)

    def _update(self, lr, wd, scale):
        c1, c2 = C.c_float(0), C.c_float(0)
        capi.call("gnnx_adam_bias_corrections", self.b1, self.b2, self.t + 1, C.byref(c1), C.byref(c2))
        capi.call("gnnx_adam_step_f32", _ptr(self._table), self._n, self._chunks, _ptr(self._arenas[0]), _ptr(self._arenas[1]), lr, self.b1,
                  self.b2, self.eps, c1.value, c2.value, wd, int(self.decoupled), scale, _stream())

    def state(self):
        """dict(m=[...], v=[...], t=t): per-tensor views of the two moment arenas, in params() order (empty before the first step)."""
        if self._bound is None:
            return dict(m=[], v=[], t=self.t)
        return dict(m=self._views(self._arenas[0]), v=self._views(self._arenas[1]), t=self.t)


class Momentum(_TableOptimizer):
    """SGD with momentum, dampening and Nesterov's form (torch.optim.SGD's update, include/gnnx.h): the buffer of the first step is the
    gradient itself."""

    def __init__(self, momentum=0.9, dampening=0.0, nesterov=False, max_grad_norm=None):
        super().__init__(max_grad_norm)
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)

    def _update(self, lr, wd, scale):
        capi.call("gnnx_momentum_step_f32", _ptr(self._table), self._n, self._chunks, _ptr(self._arenas[0]), lr, self.momentum, self.dampening,
                  int(self.nesterov), int(self.t == 0), wd, scale, _stream())

    def state(self):
        """dict(buf=[...], t=t): per-tensor views of the momentum arena, in params() order (empty before the first step)."""
        return dict(buf=[] if self._bound is None else self._views(self._arenas[0]), t=self.t)


class _Model:
    """What the trainable models share: the table `_buf` of persistent scratch buffers, one step of the model's optimiser over the
    parallel lists params() / grads() (a subclass defines both: every parameter tensor, and its gradient at the same position), and
    _view, the one way to make a second model on the same parameters.  A subclass creates `_buf = {}`, `_saved = None` and the
    optimiser's slot `_opt = [None]` in its __init__: _view hands the slot itself on, so the optimiser set on a model is the
    optimiser of every view of it, made before or after set_optimizer."""

    gather_pitch = False   # only GcnStack asks its graph (GcnStack._bind)

    def _tmp(self, key, shape, dtype=torch.float32, zero=False, gathered=False):
        """The persistent buffer `key`: the cached tensor while the shape matches, a new one otherwise (zero-filled with `zero`), on the
        parameters' device.  gathered: an [n, F] float32 matrix whose rows an aggregation gathers -- on the gather pitch
        (empty_gathered) when the model's graph wants it."""
        t = self._buf.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            dev = self.params()[0].device
            if gathered and self.gather_pitch:
                t = empty_gathered(*shape, device=dev)
            else:
                t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)
            self._buf[key] = t
        return t

    def set_optimizer(self, opt):
        """Every later step of this model and of every view of it (SageStack.on_graph, GraphClassifier.on_batch) is a step of `opt`
        (ops.Adam, ops.Momentum), with ONE state and one step count; None: back to plain SGD.  The optimiser binds to params() /
        grads() at its first step.  Returns the model.  A GraphClassifier owns the optimiser of net.params() + [W_c, b_c]; one set on
        the stack it was built from drives that stack's own steps only."""
        if opt is not None and not isinstance(opt, _TableOptimizer):
            raise TypeError(f"ops.Adam or ops.Momentum expected, got {type(opt).__name__}")
        self._opt[0] = opt
        return self

    @property
    def optimizer(self):
        return self._opt[0]

    def step(self, lr, weight_decay=0.0):
        """One step of the model's optimiser: plain SGD, a launch per tensor, unless set_optimizer chose another (one launch for all
        tensors, two with gradient clipping)."""
        opt = self._opt[0]
        if opt is not None:
            opt.step(self.params(), self.grads(), lr, weight_decay)
            return
        for p, gr in zip(self.params(), self.grads()):
            sgd_step(p, gr, lr, weight_decay)

    def _view(self, share_buf=False, **rebound):
        """A second model of this class on the SAME parameter and gradient tensors (a step through either is a step of both), with no
        saved activations, the attributes of `rebound` replaced, and either this model's buffer table itself (share_buf: the shapes
        stay) or an empty one."""
        view = object.__new__(type(self))
        view.__dict__.update(self.__dict__)   # the parameter lists themselves, not copies
        view.__dict__.update(rebound, _saved=None, _buf=self._buf if share_buf else {})
        return view


class _Stack(_Model):
    """What the three graph stacks share.  A subclass has forward(X) / backward(dOut, input_grad, have_last_bias_grad), the bias
    gradients `db`, and _bind(g): the ONE method that derives everything the class takes from its graph (g itself included) and returns
    self -- __init__ and every rebinding to another graph call it (SageStack.on_graph, GraphClassifier).  On those rest train_step /
    evaluate and the link-prediction calls (link_scores, link_grad, link_train_step, link_evaluate: an inner-product decoder on the
    stack's output), the same for every stack.

    The top gradient's buffer carries a mark in `_buf`, next to it: the selection object (a row list, a LabelledSet) outside whose rows
    the buffer is known to be zero, which is what softmax_ce_rows needs of it.  masked_grad_buffer zeroes the buffer only when the mark
    names another object; the mark is dropped when the buffer is reallocated and whenever grad_buffer() hands the buffer to a caller,
    who may write every row (softmax_ce, GraphClassifier.backward, link_grad).  Models that share `_buf` share the mark."""

    _ZERO_OUTSIDE = "zero outside"   # the mark's key in _buf; the entry keeps the selection alive, so `is` cannot match a recycled id

    def _grad(self, n=None):
        """The top gradient's buffer, [n (default g.n), dims[-1]], with the mark as it stands unless the buffer had to be reallocated."""
        key = ("G", len(self.dims) - 1)
        old = self._buf.get(key)
        G = self._tmp(key, (self.g.n if n is None else n, self.dims[-1]), gathered=True)   # gathered by the last backward aggregation
        if G is not old:
            self._buf.pop(self._ZERO_OUTSIDE, None)
        return G

    def grad_buffer(self, n=None):
        """Where the loss should write dlogits ([n (default: the graph's), dims[-1]]): softmax_ce(..., grad_out=net.grad_buffer()).  On
        the gather pitch when the model's graph wants it (GcnStack._bind): the top gradient is gathered by the last layer's backward
        aggregation."""
        self._buf.pop(self._ZERO_OUTSIDE, None)
        return self._grad(n)

    def masked_grad_buffer(self, selection):
        """The gradient buffer, zero everywhere outside the rows softmax_ce_rows writes for `selection`: zeroed when the object is first
        used and whenever the mark names another one (the rows that one wrote must become zero again)."""
        G = self._grad()
        if self._buf.get(self._ZERO_OUTSIDE) is not selection:
            G.zero_()
            self._buf[self._ZERO_OUTSIDE] = selection
        return G

    def _selected(self, selection):
        """(rows of the selection, what forward and backward are told about it)"""
        return selection, {}

    def train_step(self, X, target, rows, lr, weight_decay=0.0):
        """One step of the model's optimiser (plain SGD by default) on the selected rows: forward -> softmax_ce_rows over them (db[-1]
        from the loss kernel) -> backward without an input gradient -> step.  rows: ascending int32 rows (CsrGraph.rows_of(mask)) --
        for GcnStack a LabelledSet (CsrGraph.labelled(mask)), which also prunes the last layer's two aggregations to its rows; no other layer of any stack is pruned.  X and target in the
        graph's ROW order (g.to_new_order of vertex-order data); target is read at selected rows only.  Returns the loss tensor."""
        selection, (rows, pruned) = rows, self._selected(rows)
        logits = self.forward(X, **pruned)
        loss, G = softmax_ce_rows(logits, target, rows, colsum_out=self.db[-1], grad_out=self.masked_grad_buffer(selection))
        self.backward(G, input_grad=False, have_last_bias_grad=True, **pruned)
        self.step(lr, weight_decay)
        return loss

    def evaluate(self, X, target, rows):
        """Full forward, then (loss over `rows` as a 1-element tensor, correct predictions among them, len(rows)).  rows: ascending
        int32 rows of the graph (g.rows_of(mask) for a vertex-order validation / test mask)."""
        return _loss_and_accuracy(self.forward(X), target, rows)

    def link_scores(self, X, edges):
        """Inner-product decoder on the stack's embeddings Z = forward(X): the logit <Z[i], Z[c]> of every pair (i, c) of the EdgeSet, in
        the order of its pattern (edges.rowptr / edges.colidx) -- sddmm(edges.rowptr, edges.colidx, Z, Z)."""
        Z = self.forward(X)
        return sddmm(edges.rowptr, edges.colidx, Z, Z)

    def link_grad(self, Z, edges, ds, out=None):
        """dZ of sum_p loss_p(<Z[i_p], Z[c_p]>) from ds = dloss/dscores: row i collects ds[p] * Z[c_p] over its own entries (an
        aggregation on the pattern with vals = ds), then ds[p] * Z[i_p] over the entries that name it as a column (the transposed
        pattern with the mapped values, beta = 1).  No atomics; the order is the aggregation's own contract, the same bits every run."""
        if out is None:
            out = self.grad_buffer(Z.shape[0])
        spmm(edges.rowptr, edges.colidx, Z, out=out, vals=ds)
        spmm(edges.rowptr_t, edges.colidx_t, Z, out=out, vals=edges.to_transposed(ds), beta=1.0)
        return out

    def link_train_step(self, X, edges, lr, weight_decay=0.0):
        """One link-prediction step of the model's optimiser (plain SGD by default): forward -> pair scores (sddmm) -> bce_logits
        against edges.target -> dZ (link_grad, into grad_buffer()) -> backward without an input gradient -> step.  X in the graph's
        ROW order.  Returns the loss tensor."""
        Z = self.forward(X)
        scores = sddmm(edges.rowptr, edges.colidx, Z, Z)
        loss, ds = bce_logits(scores, edges.target)
        dZ = self.link_grad(Z, edges, ds)
        self.backward(dZ, input_grad=False)
        self.step(lr, weight_decay)
        return loss

    def link_evaluate(self, X, g, positives, m, seed, ks=(10, 50, 100)):
        """link_metrics of held-out edges: every positive (an EdgeSet or a (rowptr, colidx) pair on g's rows) against m negatives drawn
        by g.sample_negatives(m, seed, positives).  Z = forward(X); the positive scores are sddmm on the positives' pattern, the
        negative scores sddmm on (rowptr * m, neg): the entry-major layout makes a row's draws one contiguous row of that pattern, so
        the scores carry sddmm's bit contract.  An unfilled draw (-1) is scored at column 0 and skipped by the rank counts."""
        rowptr, colidx = _pattern_of(positives, "link_evaluate")
        neg, _ = g.sample_negatives(m, seed, (rowptr, colidx))
        Z = self.forward(X)
        pos_scores = sddmm(rowptr, colidx, Z, Z)
        neg_scores = sddmm(rowptr * int(m), neg.reshape(-1).clamp(min=0), Z, Z)
        return link_metrics(pos_scores, neg_scores.reshape(-1, int(m)), neg, ks)


class GcnStack(_Stack):
    """L GCN layers on one graph: h_{l+1} = act( norm (.) (A . (h_l W_l^T)) + b_l ), ReLU between layers, none after the
    last.  forward / backward / SGD step, every op a C-ABI call; activations are kept for backward.  train_step / evaluate /
    grad_buffer / masked_grad_buffer are _Stack's; the selection of train_step and masked_grad_buffer is a LabelledSet
    (CsrGraph.labelled(mask)), which forward and backward also take to prune the last layer (_selected).

    Layout for widths off the 128 grid (pad_streamed; automatic for widths >= 64 on graphs of >= 100 000 nodes: the
    products-shaped F = 100): matrices whose rows are only STREAMED by the dense products -- layer inputs / outputs Y_l, dH_l,
    W_l, dW_l -- are stored with every width rounded up to 128 floats, pad columns zero (they stay zero: the aggregations write
    the logical columns only, the products of zero columns are zero), so the products run on the LDS-DMA kernels; matrices
    whose rows are GATHERED by the aggregations -- H_l = h_l W_l^T and the gradients G_l -- keep their own width (a 512-byte
    stride there costs the gather more than the products gain).  Zero columns add exact zeros at the end of
    every fmaf chain: the logical columns have the same bits in both layouts (dW: up to how split-K cuts the rows)."""

    def __init__(self, g, dims, seed=0, device="cuda", pad_streamed=None):
        self._bind(g)
        self.dims = list(dims)
        L = len(dims) - 1
        if pad_streamed is None:
            pad_streamed = g.n >= 100_000
        self.P = [-(-d // 128) * 128 if (pad_streamed and d % 128 and d >= 64) else d for d in dims]
        self.padded = self.P != self.dims
        self.Wp = [torch.zeros((self.P[l + 1], self.P[l]), dtype=torch.float32, device=device) for l in range(L)]
        self.dWp = [torch.zeros_like(w) for w in self.Wp]
        self.W = [self.Wp[l][:dims[l + 1], :dims[l]] for l in range(L)]     # the logical matrices (views)
        self.dW = [self.dWp[l][:dims[l + 1], :dims[l]] for l in range(L)]
        for l in range(L):
            self.W[l].copy_(uniform_pm1(seed + 2 * l, (dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device))
        self.b = [torch.zeros(dims[l + 1], dtype=torch.float32, device=device) for l in range(L)]
        self.db = [torch.zeros_like(b) for b in self.b]
        self._saved = None
        self._buf = {}
        self._opt = [None]

    def _bind(self, g):
        """The matrices the aggregations GATHER rows from -- H_l = h_l W_l^T forward, the gradients G_l backward -- sit on the padded
        row pitch (gnnx_gather_row_stride) when the graph's hub ids call for it (a synthetic power-law graph in its as-generated
        vertex order: gnnx_spmm_plan_hub_ids_structured).  Every one of them is written by a kernel of this stack (the products,
        the loss: softmax_ce(grad_out=net.grad_buffer())), so the pitch costs nothing per step; same bits.  A caller's wide input
        that forward checked once is checked again on a new graph."""
        self.g = g
        self.gather_pitch = bool(g.plan is not None and g.plan_t is not None and (g.plan.hub_ids_structured() or g.plan_t.hub_ids_structured()))
        self._checked_input = None
        return self

    def params(self):
        return self.Wp + self.b   # padded storage: pads are 0 - lr * (0 + wd * 0) = 0

    def grads(self):
        return self.dWp + self.db

    def _selected(self, labelled):
        return labelled.rows, {"labelled": labelled}

    def pad_input(self, X):
        """[n, P0] zero-padded copy of the layer-0 input (call once for static features; forward() accepts its [:, :d0] view)."""
        if self.P[0] == self.dims[0]:
            return X
        Xp = torch.zeros((X.shape[0], self.P[0]), dtype=torch.float32, device=X.device)
        Xp[:, :self.dims[0]] = X
        return Xp[:, :self.dims[0]]

    def forward(self, X, labelled=None):
        """labelled (CsrGraph.labelled): the LAST layer aggregates on the row-restricted CSR -- logits rows of labelled vertices have
        the bits of the full forward, every other logits row holds the last bias (not computed).  Layers below are not pruned."""
        L = len(self.W)
        if not self.padded:
            saved, h = [], X
            for l in range(L):
                H = linear_fwd(h, self.W[l], out=self._tmp(("H", l), (X.shape[0], self.dims[l + 1]), gathered=True))
                # the ReLU between layers rides in the aggregation's epilogue: only relu(Z) is stored (its sign is the mask)
                Y = aggregate_fwd(self.g, H, self.b[l], relu_out=l + 1 < L, labelled=labelled if l + 1 == L else None)
                saved.append((h, Y))
                h = Y
            self._saved = saved
            return h
        n, d, P = X.shape[0], self.dims, self.P
        if P[0] != d[0]:
            if X.stride(0) != P[0] or X.stride(1) != 1:   # not a view of a padded buffer (pad_input): pad a copy
                X = self.pad_input(X)
            hp = torch.as_strided(X, (n, P[0]), (P[0], 1))
            if getattr(self, "_checked_input", None) != (X.data_ptr(), n):   # a caller's own wide buffer: its pad columns must be zero
                if bool(hp[:, d[0]:].any()):
                    raise ValueError("the columns behind the input's logical width must be zero (use GcnStack.pad_input)")
                self._checked_input = (X.data_ptr(), n)
        else:
            hp = X
        saved = []
        for l in range(L):
            H = linear_fwd(hp, self.Wp[l][:d[l + 1]])                 # K = P[l] (zero pads), N = d[l+1]: gathered, own width
            Yp = self._tmp(("Y", l), (n, P[l + 1]), zero=True)   # (pad columns are written once, here)
            aggregate_fwd(self.g, H, self.b[l], out=Yp[:, :d[l + 1]], relu_out=l + 1 < L, labelled=labelled if l + 1 == L else None)
            saved.append((hp, Yp))
            hp = Yp
        self._saved = saved
        return hp[:, :d[L]]

    def backward(self, dOut, fused=True, input_grad=True, have_last_bias_grad=False, labelled=None):
        """fused: the ReLU mask of the layer below and its bias gradient ride in the epilogue of dH . W
        (gnnx_gemm_relu_colsum_f32); fused=False runs them as their own passes (same G bits, db within rounding).
        input_grad=False: the stack's input is data (no requires_grad, as the reference's DataBatch features): dH . W of the
        first layer is not computed and None is returned.  have_last_bias_grad: db[L-1] was already written by the loss kernel
        (softmax_ce(..., colsum_out=net.db[-1])).  labelled (CsrGraph.labelled): dOut is zero outside the labelled rows
        (softmax_ce_rows into a zeroed buffer); the LAST layer's backward aggregation runs on the column-restricted CSR(A^T) -- same
        bits; the dense products and the layers below are not pruned."""
        G = dOut
        L = len(self.W)
        d, P = self.dims, self.P
        if not have_last_bias_grad:
            colsum(G, out=self.db[L - 1])
        for l in reversed(range(L)):
            h, Y = self._saved[l]
            if self.padded:
                # streamed: padded width.  One buffer per (padded, logical) width pair: the aggregation writes columns [:d] only, so two
                # layers whose widths differ but round to the same 128-float bucket must not share pad columns (a narrower layer
                # would inherit the wider one's values there, and dW / W pads would stop being zero)
                dH = self._tmp(("dH", P[l + 1], d[l + 1]), (G.shape[0], P[l + 1]), zero=True)
                aggregate_bwd(self.g, G, out=dH[:, :d[l + 1]], labelled=labelled if l + 1 == L else None)
                Wl, hl = self.Wp[l][:, :d[l]], h[:, :d[l]]            # [P_out, d_in] (ld P_in); the layer input, logical width
                gemm(dH, h, transA=True, out=self.dWp[l])             # dW_l = dH^T . h on the padded widths
            else:
                dH = aggregate_bwd(self.g, G, labelled=labelled if l + 1 == L else None)
                Wl, hl = self.W[l], h
                gemm(dH, h, transA=True, out=self.dW[l])          # dW_l = dH^T . h
            if l == 0:
                G = gemm(dH, Wl) if input_grad else None             # dX of the first layer: no ReLU below it
            elif fused:
                # h = Y_{l-1} = relu output of the layer below; G_{l-1} is gathered by that layer's backward aggregation
                G, _ = gemm_relu_colsum(dH, Wl, hl, out=self._tmp(("G", l), (dH.shape[0], Wl.shape[1]), gathered=True), colsum_out=self.db[l - 1])
            else:
                G = gemm(dH, Wl)
                G, _, _ = bn_relu_bwd(hl, hl, G, relu=True)
                colsum(G, out=self.db[l - 1])
        return G

    def _field_logits(self, X, field):
        """[len(field.rows[L]), C] logits of the field's unique query rows (compact row k = graph row field.rows[L][k]), each layer a
        plain product and aggregation on the compact matrices of the field.  Same layout rules as forward (padded: streamed
        matrices on the 128-float widths, gathered H on its own width), buffers of its own: _saved and _buf are not touched."""
        L = len(self.W)
        if not isinstance(field, ReceptiveField) or field.n_layers != L:
            raise ValueError(f"the stack has {L} layers, the receptive field was built for {getattr(field, 'n_layers', None)}")
        if field.n != self.g.n or X.shape[0] != self.g.n or X.shape[1] != self.dims[0]:
            raise ValueError("X must be the full [n, d0] input of the graph the field was built on")
        d, P, dev = self.dims, self.P, X.device

        def rows_buf(m, width):   # [m, width] zero-filled when a pad exists, on a buffer of at least one row (a device pointer even for m = 0)
            make = torch.zeros if self.padded else torch.empty
            return make((max(m, 1), width), dtype=torch.float32, device=dev)[:m]

        m = int(field.rows[0].numel())
        hp = rows_buf(m, P[0])
        if m:
            gather_rows(X, field.rows[0], out=hp[:, :d[0]])     # the only read of the input: rows Q_0
        for l in range(1, L + 1):
            m_in, m_out = m, int(field.rows[l].numel())
            if m_in:
                H = linear_fwd(hp, self.Wp[l - 1][:d[l]])        # K = P[l-1] (zero pads), N = d[l]: gathered, own width
            else:   # an empty frontier: a block of no entries over one row nobody reads (the aggregation wants a device pointer)
                H = torch.zeros((1, d[l]), dtype=torch.float32, device=dev)
            Yp = rows_buf(m_out, P[l])
            if m_out:
                rp, ci = field.block[l]
                spmm(rp, ci, H, out=Yp[:, :d[l]], rowscale=field.norm[l], bias=self.b[l - 1], plan=field.plan[l], n_rows=m_out,
                     relu_out=l < L)
            hp, m = Yp, m_out
        return hp[:, :d[L]]

    def predict(self, X, field):
        """Logits [len(query), C] of the field's query, one row per query entry in the caller's order, computed on the field's compact
        matrices: bit for bit forward(X)[field.query_rows].  X: the full [n, d0] input in row order, as forward takes it; only rows
        field.rows[0] are read.  There is no fallback to the full forward: field.rows / field.nnz say what the call costs."""
        logits = self._field_logits(X, field)
        if field.n_query == 0:
            return torch.empty((0, self.dims[-1]), dtype=torch.float32, device=X.device)
        return gather_rows(logits, field.query_pos)

    def evaluate_field(self, X, target, field):
        """evaluate(X, target, field.rows[L]) from predict's compact logits: (loss over the query's rows as a 1-element tensor, correct
        predictions among them, their number) -- the same loss bits and the same count.  target: [n] in row order, read at the
        query's rows only."""
        logits = self._field_logits(X, field)
        rows = field.rows[len(self.W)]
        t = target.reshape(-1)[rows.long()].to(torch.int32).contiguous()
        return _loss_and_accuracy(logits, t, field.compact_rows)


class _AttentionStack(_Stack):
    """What the attention stacks (GatStack, Gatv2Stack) share beyond _Stack: the heads of every layer, the transpose map of the graph,
    and the three steps that ask how many heads a layer has or which pattern a value array is ordered by."""

    @staticmethod
    def _heads_per_layer(dims, heads):
        L = len(dims) - 1
        heads = [1] * L if heads is None else list(heads)
        if len(heads) != L or any(int(k) != k or k < 1 for k in heads):
            raise ValueError(f"heads must list {L} positive integers, one per layer, got {heads}")
        bad = [l for l in range(L) if dims[l + 1] % heads[l]]
        if bad:
            raise ValueError(f"layer {bad[0]}: {dims[bad[0] + 1]} features do not split into {heads[bad[0]]} heads")
        return [int(k) for k in heads]

    def _bind(self, g):
        self.g = g
        self.map_t = g.attention_map()
        return self

    def _aggregate(self, l, X, vals, transposed=False, **epilogue):
        """sum_p vals[p, h] * X[c_p, slab h] over the rows of the pattern (of the transposed pattern: vals in its order).  One head: the
        planned kernel, which splits hub rows; several: spmm_heads, which has no plan."""
        g = self.g
        rowptr, colidx, plan = (g.rowptr_t, g.colidx_t, g.plan_t) if transposed else (g.rowptr, g.colidx, g.plan)
        if self.heads[l] == 1:
            return spmm(rowptr, colidx, X, vals=vals.reshape(-1), plan=plan, **epilogue)
        return spmm_heads(rowptr, colidx, X, vals, self.heads[l], **epilogue)

    def _vals_grad(self, l, G, H):
        """dL/dalpha [nnz, Hh], the aggregation's value gradient.  One head: sddmm, which prefetches the next batch of columns."""
        g = self.g
        if self.heads[l] == 1:
            return spmm_vals_grad(g.rowptr, g.colidx, G, H).reshape(-1, 1)
        return sddmm_heads(g.rowptr, g.colidx, G, H, self.heads[l])

    def _to_transposed(self, vals, out):
        if self.g.nnz:
            gather_rows(vals.reshape(int(vals.shape[0]), -1), self.map_t, out=out.reshape(int(out.shape[0]), -1))
        return out


class GatStack(_AttentionStack):
    """L graph-attention layers (GAT, Velickovic et al. 2018) on one graph, the surface of GcnStack.  Layer l has heads[l] heads of width
    D = dims[l+1] / heads[l]; per head
        H = h W^T;   el = H a_l,  er = H a_r;   alpha_ic = softmax over the stored entries c of row i of leaky_relu(el_i + er_c);
        h' = act( sum_c alpha_ic H_c + b ),  ReLU between layers, none after the last,
    and the layer's output is the concatenation of its heads (the usual last layer is one head; head averaging and attention dropout are
    not implemented).  heads=None means one head in every layer.  Row i attends over its STORED columns -- the direction of the
    project's aggregation.  forward / backward / step / train_step / evaluate; every operation is a C-ABI call.  No atomics; the same
    bits every run.

    There is ONE layer path.  The attention vectors ride as one [2 Hh, Hh D] matrix A that is zero outside its blocks (row h: a_l of head
    h in the head's columns, row Hh + h: a_r; for one head the plain [2, d] matrix [a_l; a_r]), so ER = H A^T is [n, 2 Hh] with el in the
    left half and er in the right, and the backward's two products with dER = [del der] work for any number of heads; dA is masked to
    the blocks (A_mask).  The softmax and the row sums are the multi-head calls (edge_softmax_heads, edge_softmax_heads_bwd,
    csr_rowsum_heads), which write both halves of dER in place; everything that flows back to a column's vertex goes through the
    transposed pattern with g.attention_map().  Only two steps ask how many heads a layer has (_aggregate, _vals_grad): a one-head layer
    keeps the planned aggregation (spmm with g.plan / g.plan_t: a hub row is split) and the prefetching edge
    scores (spmm_vals_grad), a layer of several heads reads the pattern once for all of them (spmm_heads, sddmm_heads).

    The stack takes any CsrGraph that has a transposed CSR and is not relabelled.  CsrGraph.from_coo strips the diagonal; the paper's
    self attention wants every vertex in its own row, a pattern with the whole diagonal:
        w = torch.ones(src.numel(), device=src.device)
        rp, ci, _ = csr_from_coo_weighted(src, dst, w, n, DIAG_FILL)          # the values are discarded
        rp_t, ci_t, _ = csr_from_coo_weighted(dst, src, w, n, DIAG_FILL)
        g = CsrGraph(n, rp, ci, rp_t, ci_t)                                   # g.make_plans(...) for a power-law graph
    A vertex without entries (only possible without the diagonal) has an empty softmax: its row is the bias alone."""

    def __init__(self, g, dims, negative_slope=0.2, seed=0, device="cuda", heads=None):
        self._bind(g)
        self.dims = list(dims)
        self.negative_slope = float(negative_slope)
        L = len(dims) - 1
        self.heads = self._heads_per_layer(dims, heads)
        self.W = [uniform_pm1(seed + 2 * l, (dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device) for l in range(L)]
        self.A, self.A_mask = [], []
        for l, Hh in enumerate(self.heads):   # [a_l; a_r] drawn as one [2, dims[l+1]] matrix, laid out in the blocks of the [2 Hh, Hh D] one
            D = dims[l + 1] // Hh
            block = torch.kron(torch.eye(Hh, dtype=torch.float32, device=device), torch.ones((1, D), dtype=torch.float32, device=device))
            mask = torch.cat([block, block]).contiguous()
            draw = uniform_pm1(seed + 2 * l + 1, (2, dims[l + 1]), scale=D ** -0.5, device=device)
            self.A.append((torch.cat([draw[0:1].expand(Hh, -1), draw[1:2].expand(Hh, -1)]) * mask).contiguous())
            self.A_mask.append(mask)
        self.b = [torch.zeros(dims[l + 1], dtype=torch.float32, device=device) for l in range(L)]
        self.dW = [torch.zeros_like(w) for w in self.W]
        self.dA = [torch.zeros_like(a) for a in self.A]
        self.db = [torch.zeros_like(b) for b in self.b]
        self._saved = None
        self._buf = {}
        self._opt = [None]

    def params(self):
        return self.W + self.A + self.b

    def grads(self):
        return self.dW + self.dA + self.db

    def attention(self, H, l):
        """(ER, alpha) of layer l from H = h W_l^T: ER = H A^T as [n, 2 Hh] (el of head h in column h, er in column Hh + h), alpha entry-major
        [nnz, Hh] = edge_softmax_heads(rowterm = ER[:, :Hh], colterm = ER[:, Hh:])."""
        g, Hh = self.g, self.heads[l]
        ER = gemm(H, self.A[l], transB=True)
        alpha = edge_softmax_heads(g.rowptr, g.colidx, Hh, rowterm=ER[:, :Hh], colterm=ER[:, Hh:], negative_slope=self.negative_slope)
        return ER, alpha

    def forward(self, X):
        L = len(self.W)
        saved, h = [], X
        for l in range(L):
            H = linear_fwd(h, self.W[l])
            ER, alpha = self.attention(H, l)
            # the ReLU between layers rides in the aggregation's epilogue: only relu(Z) is stored (its sign is the mask)
            Y = self._aggregate(l, H, alpha, bias=self.b[l], relu_out=l + 1 < L)
            saved.append((h, H, ER, alpha, Y))
            h = Y
        self._saved = saved
        return h

    def backward(self, dOut, input_grad=True, have_last_bias_grad=False):
        """dW, dA (masked to its blocks) and db of every layer from dOut = dL/dlogits; returns dL/dX (None with input_grad=False).
        have_last_bias_grad: db[L-1] was already written by the loss kernel (softmax_ce_rows(..., colsum_out=net.db[-1]))."""
        g, L, n = self.g, len(self.W), self.g.n
        G = dOut
        if not have_last_bias_grad:
            colsum(G, out=self.db[L - 1])
        for l in reversed(range(L)):
            h, H, ER, alpha, _ = self._saved[l]
            Hh = self.heads[l]
            dalpha = self._vals_grad(l, G, H)
            dER = self._tmp(("dER", Hh), (n, 2 * Hh))                                     # left half: del, right half: der
            dt, _ = edge_softmax_heads_bwd(g.rowptr, g.colidx, Hh, alpha, dalpha, rowterm=ER[:, :Hh], colterm=ER[:, Hh:],
                                           negative_slope=self.negative_slope, drowterm_out=dER[:, :Hh])
            vals_t = self._tmp(("vals_t", Hh), (g.nnz, Hh))
            self._to_transposed(dt, vals_t)
            csr_rowsum_heads(g.rowptr_t, vals_t, out=dER[:, Hh:])                         # der: what flows back to a column's vertex
            self._to_transposed(alpha, vals_t)
            dH = self._aggregate(l, G, vals_t, transposed=True)                           # through the aggregated rows
            gemm(dER, self.A[l], out=dH, beta=1.0)                                        # + [del der] . A, through ER
            gemm(dER, H, transA=True, out=self.dA[l])
            if Hh > 1:   # the entries outside the blocks are not parameters (one head: the mask is all ones)
                binary("mul", self.dA[l], self.A_mask[l], out=self.dA[l])
            gemm(dH, h, transA=True, out=self.dW[l])
            if l == 0:
                G = gemm(dH, self.W[l]) if input_grad else None
            else:   # h = relu output of the layer below: its mask and the bias gradient in the product's epilogue
                G, _ = gemm_relu_colsum(dH, self.W[l], h, colsum_out=self.db[l - 1])
        return G


class Gatv2Stack(_AttentionStack):
    """L GATv2 layers (Brody, Alon, Yahav 2022: dynamic attention) on one graph, the surface and the graph requirements of GatStack.
    Layer l has heads[l] heads of width D = dims[l+1] / heads[l]; per head
        Hl = h W_l^T,  Hr = h W_r^T;   e_ic = a . leaky_relu(Hl_i + Hr_c);   alpha_ic = softmax of e over the stored entries c of row i;
        h' = act( sum_c alpha_ic Hr_c + b ),  ReLU between layers, none after the last,
    the heads concatenated.  The non-linearity sits INSIDE the sum over features, so two rows that store the same columns may rank them
    differently, which GAT's leaky_relu(el_i + er_c) cannot.  heads=None means one head in every layer.  share_weights: W_l is W_r, one
    product, one weight whose gradient is the sum of both.

    The two weights of a layer ride as ONE parameter W[l] = [W_l; W_r] of shape [2 out, in] (W_l(l) / W_r(l) are its halves; with
    share_weights W[l] is [out, in] and both are W[l] itself): one product gives [Hl | Hr] as [n, 2 out], the score and the aggregation
    take the halves with ld = 2 out, the backward writes [dHl | dHr] into one [n, 2 out] buffer, and dW[l] and dh are one product each
    as in GatStack.  a[l] is a [dims[l+1]] vector, head h's vector in its slab.  The score and its two backward passes are gatv2_scores /
    gatv2_scores_bwd; the softmax runs on the given scores with slope 1; the aggregation, its value gradient and the transposed order are
    GatStack's own steps (a one-head layer keeps the planned spmm and the prefetching sddmm).  da = colsum(T) with T from the forward-
    pattern backward pass.  No atomics; the same bits every run."""

    def __init__(self, g, dims, negative_slope=0.2, seed=0, device="cuda", heads=None, share_weights=False):
        self._bind(g)
        self.dims = list(dims)
        self.negative_slope = float(negative_slope)
        self.share_weights = bool(share_weights)
        L = len(dims) - 1
        self.heads = self._heads_per_layer(dims, heads)
        k = 1 if self.share_weights else 2
        self.W = [uniform_pm1(seed + 2 * l, (k * dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device) for l in range(L)]
        self.a = [uniform_pm1(seed + 2 * l + 1, (dims[l + 1],), scale=(dims[l + 1] // self.heads[l]) ** -0.5, device=device) for l in range(L)]
        self.b = [torch.zeros(dims[l + 1], dtype=torch.float32, device=device) for l in range(L)]
        self.dW = [torch.zeros_like(w) for w in self.W]
        self.da = [torch.zeros_like(a) for a in self.a]
        self.db = [torch.zeros_like(b) for b in self.b]
        self._saved = None
        self._buf = {}
        self._opt = [None]

    def params(self):
        return self.W + self.a + self.b

    def grads(self):
        return self.dW + self.da + self.db

    def _halves(self, M, l):
        """(left, right) of a layer's [., out] or [., 2 out] matrix along its columns: the same matrix twice with share_weights."""
        out = self.dims[l + 1]
        return (M, M) if self.share_weights else (M[:, :out], M[:, out:])

    def W_l(self, l):
        return self.W[l] if self.share_weights else self.W[l][:self.dims[l + 1]]

    def W_r(self, l):
        return self.W[l] if self.share_weights else self.W[l][self.dims[l + 1]:]

    def attention(self, Hl, Hr, l):
        """(e, alpha) of layer l, both entry-major [nnz, Hh]: e = gatv2_scores(Hl, Hr, a[l]), alpha = edge_softmax_heads(scores = e)."""
        g, Hh = self.g, self.heads[l]
        e = gatv2_scores(g.rowptr, g.colidx, Hl, Hr, self.a[l], Hh, negative_slope=self.negative_slope)
        return e, edge_softmax_heads(g.rowptr, g.colidx, Hh, scores=e, negative_slope=1.0)

    def forward(self, X):
        L = len(self.W)
        saved, h = [], X
        for l in range(L):
            Hlr = linear_fwd(h, self.W[l])
            Hl, Hr = self._halves(Hlr, l)
            e, alpha = self.attention(Hl, Hr, l)
            Y = self._aggregate(l, Hr, alpha, bias=self.b[l], relu_out=l + 1 < L)   # only relu(Z) is stored (its sign is the mask)
            saved.append((h, Hlr, e, alpha, Y))
            h = Y
        self._saved = saved
        return h

    def backward(self, dOut, input_grad=True, have_last_bias_grad=False):
        """dW, da and db of every layer from dOut = dL/dlogits; returns dL/dX (None with input_grad=False).  have_last_bias_grad: db[L-1]
        was already written by the loss kernel (softmax_ce_rows(..., colsum_out=net.db[-1]))."""
        g, L, n = self.g, len(self.W), self.g.n
        G = dOut
        if not have_last_bias_grad:
            colsum(G, out=self.db[L - 1])
        for l in reversed(range(L)):
            h, Hlr, e, alpha, _ = self._saved[l]
            Hl, Hr = self._halves(Hlr, l)
            Hh, out = self.heads[l], self.dims[l + 1]
            dalpha = self._vals_grad(l, G, Hr)
            de, _ = edge_softmax_heads_bwd(g.rowptr, g.colidx, Hh, alpha, dalpha, scores=e, negative_slope=1.0,
                                           drowterm_out=self._tmp(("drow", Hh), (n, Hh)), dt_out=self._tmp(("de", Hh), (g.nnz, Hh)))
            dHlr = self._tmp(("dH", l), tuple(Hlr.shape))                                  # [dHl | dHr]; one matrix with share_weights
            dHl, dHr = self._halves(dHlr, l)
            vals_t = self._tmp(("vals_t", Hh), (g.nnz, Hh))
            self._to_transposed(alpha, vals_t)
            self._aggregate(l, G, vals_t, transposed=True, out=dHr)                        # through the aggregated rows
            gatv2_scores_bwd(g.rowptr_t, g.colidx_t, de, Hr, Hl, self.a[l], Hh, negative_slope=self.negative_slope, entry_map=self.map_t,
                             out=dHr, beta=1.0)                                            # + through the score's column side
            gatv2_scores_bwd(g.rowptr, g.colidx, de, Hl, Hr, self.a[l], Hh, negative_slope=self.negative_slope, out=dHl,
                             beta=1.0 if self.share_weights else 0.0, T_out=self._tmp(("T", l), (n, out)))   # the row side, and T
            colsum(self._buf[("T", l)], out=self.da[l])
            gemm(dHlr, h, transA=True, out=self.dW[l])
            if l == 0:
                G = gemm(dHlr, self.W[l]) if input_grad else None
            else:   # h = relu output of the layer below: its mask and the bias gradient in the product's epilogue
                G, _ = gemm_relu_colsum(dHlr, self.W[l], h, colsum_out=self.db[l - 1])
        return G


def relu_mask(Y, dY, out=None):
    """out = dY where Y > 0, else 0 -- ReLU's backward from its stored output (gnnx_bn_relu_bwd_f32 without statistics)."""
    N, F = Y.shape
    out = torch.empty_like(dY) if out is None else out
    ws, wsb = _scratch("gnnx_bn_workspace", N, F, device=Y.device, tag="bn")
    capi.call("gnnx_bn_relu_bwd_f32", _ptr(Y), _ld(Y), _ptr(Y), _ld(Y), _ptr(dY), _ld(dY), N, F, None, None, 0.0, None, None, 1, _ptr(out), _ld(out),
              None, None, _ptr(ws), wsb, _stream())
    return out


class SageStack(_Stack):
    """L GraphSAGE layers (Hamilton et al. 2017) on one graph, the surface of GatStack: the vertex keeps a weight of its own,
        M = agg_j h_j over the STORED columns j of row i;   h' = act( h W_s^T + M W_n^T + b ),  ReLU between layers, none after the last.
    aggr="mean": M = inv_deg (.) (A . h) with inv_deg[i] = 1 / deg_i (one correctly rounded division; 0 for an empty row) -- the planned
    aggregation (spmm with rowscale, g.plan) forward, and spmm on CSR(A^T) with colscale = inv_deg (g.plan_t) backward: existing
    kernels with existing bits, so a relabelled graph is fine.  aggr="max": M, arg = spmm_reduce(h) forward with arg kept per layer, and
    spmm_reduce_bwd through g.attention_map() backward -- which refuses a relabelled graph and one without a transposed CSR, with
    GatStack's GnnxError.  An empty row aggregates to zero: its output is h W_s^T + b.
    forward / backward / step / train_step / evaluate / grad_buffer, and on_graph for steps on a sampled graph; every operation of forward and backward is a C-ABI call (the
    aggregation, the dense products, the bias add, the ReLU and its mask).  No atomics on any value; the same bits every run.
    predict / batch_step run on a SampledField (g.sampled_field(seeds, fanouts, seed)): a mini-batch at the cost of its field."""

    def __init__(self, g, dims, aggr="mean", seed=0, device="cuda"):
        if aggr not in ("mean", "max"):
            raise ValueError(f"aggr must be 'mean' or 'max', got {aggr!r}")
        self.dims, self.aggr = list(dims), aggr
        L = len(dims) - 1
        self._bind(g)
        self.W_s = [uniform_pm1(seed + 2 * l, (dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device) for l in range(L)]
        self.W_n = [uniform_pm1(seed + 2 * l + 1, (dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device) for l in range(L)]
        self.b = [torch.zeros(dims[l + 1], dtype=torch.float32, device=device) for l in range(L)]
        self.dW_s = [torch.zeros_like(w) for w in self.W_s]
        self.dW_n = [torch.zeros_like(w) for w in self.W_n]
        self.db = [torch.zeros_like(b) for b in self.b]
        self._saved = None
        self._buf = {}
        self._opt = [None]

    def _bind(self, g):
        """What the stack holds of the graph itself: the transpose map (max) or 1 / deg (mean)."""
        self.g = g
        if self.aggr == "max":
            self.map_t = g.attention_map()
        else:
            self.inv_deg = _inv_deg(g.rowptr)
        return self

    def params(self):
        return self.W_s + self.W_n + self.b

    def grads(self):
        return self.dW_s + self.dW_n + self.db

    def on_graph(self, g):
        """This stack on another graph over the same vertices -- a sample of its neighbourhoods: a SageStack that SHARES this one's
        parameters, gradients and scratch buffers (the same tensors and the same table, the gradient buffer's zeroed-rows mark
        included: a step through either is a step of both) and has its own inv_deg / map_t.  The training surface of neighbour sampling:
            net.on_graph(g.sample_neighbors(k, seed=epoch)).train_step(X, target, rows, lr)
        while net.evaluate(...) keeps running on the full graph."""
        if g.n != self.g.n:
            raise ValueError(f"the graph has {g.n} vertices, the stack was built for {self.g.n}")
        return self._view(share_buf=True)._bind(g)

    def _aggregate(self, l, h):
        """(M, arg) of layer l: the neighbourhood's mean (arg None) or its maximum with the winning entries."""
        g = self.g
        M = self._tmp(("M", l), (g.n, self.dims[l]))
        if self.aggr == "mean":
            return spmm(g.rowptr, g.colidx, h, out=M, rowscale=self.inv_deg, plan=g.plan), None
        return spmm_reduce(g.rowptr, g.colidx, h, op="max", out=M, arg_out=self._tmp(("arg", l), (g.n, self.dims[l]), torch.int32))

    def _aggregate_bwd(self, l, dM, arg, out):
        """out += the aggregation's gradient with respect to h."""
        g = self.g
        if self.aggr == "mean":
            if g.rowptr_t is None:
                raise capi.GnnxError(-1, "SageStack", "the graph has no transposed CSR (from_coo(..., transpose=True))")
            return spmm(g.rowptr_t, g.colidx_t, dM, out=out, colscale=self.inv_deg, beta=1.0, plan=g.plan_t)
        return spmm_reduce_bwd(g.rowptr_t, g.colidx_t, self.map_t, arg, dM, out=out, beta=1.0)

    def forward(self, X):
        L, n = len(self.W_s), self.g.n
        saved, h = [], X
        for l in range(L):
            M, arg = self._aggregate(l, h)
            Z = gemm(h, self.W_s[l], transB=True, out=self._tmp(("Z", l), (n, self.dims[l + 1])))
            gemm(M, self.W_n[l], transB=True, out=Z, beta=1.0)
            Y = self._tmp(("Y", l), (n, self.dims[l + 1]))
            bias_add(Z, self.b[l], out=Y)
            if l + 1 < L:   # only relu(Z + b) is kept: its sign is the mask
                bn_relu_fwd(Y, relu=True, out=Y)
            saved.append((h, M, arg, Y))
            h = Y
        self._saved = saved
        return h

    def backward(self, dOut, input_grad=True, have_last_bias_grad=False):
        """dW_s, dW_n and db of every layer from dOut = dL/dlogits; returns dL/dX (None with input_grad=False).
        have_last_bias_grad: db[L-1] was already written by the loss kernel (softmax_ce_rows(..., colsum_out=net.db[-1]))."""
        L, n = len(self.W_s), self.g.n
        G = dOut
        if not have_last_bias_grad:
            colsum(G, out=self.db[L - 1])
        for l in reversed(range(L)):
            h, M, arg, _ = self._saved[l]
            gemm(G, h, transA=True, out=self.dW_s[l])
            gemm(G, M, transA=True, out=self.dW_n[l])
            if l == 0 and not input_grad:
                return None
            dM = gemm(G, self.W_n[l], out=self._tmp(("dM", l), (n, self.dims[l])))
            dh = gemm(G, self.W_s[l], out=self._tmp(("dh", l), (n, self.dims[l])))     # through the vertex itself
            self._aggregate_bwd(l, dM, arg, dh)                                        # + through its neighbourhood
            if l == 0:
                return dh
            G = relu_mask(h, dh, out=self._tmp(("G", l), (n, self.dims[l])))           # h = relu output of the layer below
            colsum(G, out=self.db[l - 1])
        return G

    # ---- mini-batch steps on a SampledField: compact matrices of their own, neither _saved nor _buf is touched ----
    def _field_forward(self, X, field):
        """[(h, Hs, M, arg, Y)] per layer on the field's compact matrices: h the layer's input on rows[l], Hs = its rows self_pos (the
        vertices themselves), M / arg the aggregation over block l + 1, Y the output on rows[l + 1].  The operations are forward's,
        row for row: a block row holds the entries of the sampled graph's row in stored order and every product is row-local."""
        L = len(self.W_s)
        if not isinstance(field, SampledField) or field.n_layers != L:
            raise ValueError(f"the stack has {L} layers, the sampled field was built for {getattr(field, 'n_layers', None)}")
        if field.n != self.g.n or X.shape[0] != self.g.n or X.shape[1] != self.dims[0]:
            raise ValueError("X must be the full [n, d0] input of the graph the field was built on")
        if field.n_query == 0:
            raise ValueError("the field has no seeds")
        h = gather_rows(X, field.rows[0])     # the only read of the input: rows Q_0
        saved = []
        for l in range(L):
            (rp, ci), m_out = field.block[l + 1], int(field.rows[l + 1].numel())
            if self.aggr == "mean":
                M, arg = spmm(rp, ci, h, rowscale=field.inv_deg[l + 1], n_rows=m_out), None
            else:
                M, arg = spmm_reduce(rp, ci, h, op="max")
            Hs = gather_rows(h, field.self_pos[l + 1])
            Z = gemm(Hs, self.W_s[l], transB=True)
            gemm(M, self.W_n[l], transB=True, out=Z, beta=1.0)
            Y = bias_add(Z, self.b[l], out=Z)
            if l + 1 < L:
                bn_relu_fwd(Y, relu=True, out=Y)
            saved.append((h, Hs, M, arg, Y))
            h = Y
        return saved

    def predict(self, X, field):
        """Logits [len(seeds), C] of a SampledField's seeds, one row per seed in the caller's order, from the field's compact matrices.
        X: the full [n, d0] input in row order; only rows field.rows[0] are read.  With per-layer seeds [s] * L and fanouts [k] * L the
        field is the L-hop field of g.sample_neighbors(k, s) and the result is bit for bit on_graph(that graph).forward(X) at the seeds.
        Buffers of its own: a call between forward and backward leaves the step's results as they are."""
        return gather_rows(self._field_forward(X, field)[-1][4], field.query_pos)

    def batch_step(self, X, target, field, lr, weight_decay=0.0):
        """One step of the model's optimiser on a mini-batch: forward on the field, softmax_ce over all compact rows of rows[L] (the
        batch's unique vertices; db[L-1] from the loss kernel), backward on the blocks into dW_s / dW_n / db, step.  X and target in the
        graph's ROW order; target is read at rows[L] only.  Returns the loss tensor.  The training surface of mini-batches:
            for it, batch in enumerate(batches): net.batch_step(X, target, g.sampled_field(batch, [10, 10], seed=it), lr)
        The gradients are those of the loss on the sampled field, summed over its compact rows -- another split-K sum than a full-graph
        step's, so no bits are shared with train_step; every run of the same schedule gives the same bits."""
        L = len(self.W_s)
        saved = self._field_forward(X, field)
        t = target.reshape(-1)[field.rows[L].long()].to(torch.int32).contiguous()
        loss, G = softmax_ce(saved[-1][4], t, colsum_out=self.db[L - 1])
        for l in reversed(range(L)):
            h, Hs, M, arg, _ = saved[l]
            gemm(G, Hs, transA=True, out=self.dW_s[l])
            gemm(G, M, transA=True, out=self.dW_n[l])
            if l == 0:
                break
            dM = gemm(G, self.W_n[l])
            dh = torch.zeros_like(h)
            scatter_add_rows(gemm(G, self.W_s[l]), field.self_pos[l + 1], dh)         # through the vertex itself (self_pos is injective)
            rpt, cit = field.block_t[l + 1]
            if self.aggr == "mean":                                                      # + through its sampled neighbourhood
                spmm(rpt, cit, dM, out=dh, colscale=field.inv_deg[l + 1], beta=1.0)
            else:
                spmm_reduce_bwd(rpt, cit, field.map_t(l + 1), arg, dM, out=dh, beta=1.0)
            G = relu_mask(h, dh)                                                         # h = relu output of the layer below
            colsum(G, out=self.db[l - 1])
        self.step(lr, weight_decay)
        return loss


class EdgeConvStack(_Stack):
    """L EdgeConv layers (Wang et al. 2019, DGCNN) with the surface of SageStack.  The paper's layer is
        h'_i = max_j ReLU( Theta (h_j - h_i) + Phi h_i )          over the neighbours j of i.
    ReLU is monotone and Phi h_i - Theta h_i does not depend on j, so this equals ReLU( (Phi - Theta) h_i + max_j Theta h_j ): the stack
    holds W_s = Phi - Theta and W_n = Theta, and the transform runs once per VERTEX, not once per edge:
        T = h W_n^T;   M, arg = spmm_reduce(g_l, T, "max")  (an empty row gives 0);   Y = h W_s^T + M + b,
    ReLU between layers, none after the last.  Backward per layer: db = colsum(dY), dW_s = dY^T h, dh = dY W_s,
    dT = spmm_reduce_bwd(g_l^T, map_t, arg, dY), dW_n = dT^T h, dh += dT W_n.
    k=None: every layer runs on the bound graph (its attention_map() must build: no relabelling, a transposed CSR).  An integer k
    (1 .. 64): the graph of layer l is rebuilt from that layer's INPUT, knn_graph(h, k, g.graph_ptr, loop=False) -- the bound graph
    only says which rows belong together (GraphBatch.of_points) -- and the graphs of the last forward are kept in net.graphs.  No
    gradient flows through the selection, as in DGCNN.
    forward / backward / step / train_step / evaluate / grad_buffer / on_graph, and use under GraphClassifier / on_batch.  Every
    operation is a C-ABI call; no atomics on any value; the same bits every run."""

    def __init__(self, g, dims, k=None, seed=0, device="cuda"):
        if k is not None and not 1 <= int(k) <= KNN_MAX_K:
            raise ValueError(f"k must be None or 1 .. {KNN_MAX_K}, got {k!r}")
        self.dims, self.k = list(dims), None if k is None else int(k)
        L = len(dims) - 1
        self.graphs = None
        self._bind(g)
        self.W_s = [uniform_pm1(seed + 2 * l, (dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device) for l in range(L)]
        self.W_n = [uniform_pm1(seed + 2 * l + 1, (dims[l + 1], dims[l]), scale=dims[l] ** -0.5, device=device) for l in range(L)]
        self.b = [torch.zeros(dims[l + 1], dtype=torch.float32, device=device) for l in range(L)]
        self.dW_s = [torch.zeros_like(w) for w in self.W_s]
        self.dW_n = [torch.zeros_like(w) for w in self.W_n]
        self.db = [torch.zeros_like(b) for b in self.b]
        self._saved = None
        self._buf = {}
        self._opt = [None]

    def _bind(self, g):
        """What the stack holds of the graph itself: the transpose map of a fixed graph; of a dynamic one only the row ownership."""
        self.g = g
        self.graphs = None
        self.map_t = g.attention_map() if self.k is None else None
        return self

    def params(self):
        return self.W_s + self.W_n + self.b

    def grads(self):
        return self.dW_s + self.dW_n + self.db

    def on_graph(self, g):
        """This stack on another graph over the same vertices (SageStack.on_graph): shared parameters, gradients and scratch buffers."""
        if g.n != self.g.n:
            raise ValueError(f"the graph has {g.n} vertices, the stack was built for {self.g.n}")
        return self._view(share_buf=True)._bind(g)

    def _layer_graph(self, h):
        if self.k is None:
            return self.g
        return knn_graph(h, self.k, getattr(self.g, "graph_ptr", None), loop=False, transpose=True, norm=False)

    def forward(self, X):
        L, n = len(self.W_s), self.g.n
        saved, graphs, h = [], [], X
        for l in range(L):
            gl = self._layer_graph(h)
            T = gemm(h, self.W_n[l], transB=True, out=self._tmp(("T", l), (n, self.dims[l + 1])))
            M, arg = spmm_reduce(gl.rowptr, gl.colidx, T, op="max", out=self._tmp(("M", l), (n, self.dims[l + 1])),
                                 arg_out=self._tmp(("arg", l), (n, self.dims[l + 1]), torch.int32))
            Z = gemm(h, self.W_s[l], transB=True, out=self._tmp(("Z", l), (n, self.dims[l + 1])))
            axpy(1.0, M, Z)
            Y = bias_add(Z, self.b[l], out=self._tmp(("Y", l), (n, self.dims[l + 1])))
            if l + 1 < L:   # only relu(Z + b) is kept: its sign is the mask
                bn_relu_fwd(Y, relu=True, out=Y)
            saved.append((h, M, arg, Y))
            graphs.append(gl)
            h = Y
        self._saved, self.graphs = saved, graphs
        return h

    def backward(self, dOut, input_grad=True, have_last_bias_grad=False):
        """dW_s, dW_n and db of every layer from dOut = dL/dlogits; returns dL/dX (None with input_grad=False).
        have_last_bias_grad: db[L-1] was already written by the loss kernel (softmax_ce_rows(..., colsum_out=net.db[-1]))."""
        L, n = len(self.W_s), self.g.n
        G = dOut
        if not have_last_bias_grad:
            colsum(G, out=self.db[L - 1])
        for l in reversed(range(L)):
            h, _, arg, _ = self._saved[l]
            gl = self.graphs[l]
            map_t = self.map_t if self.k is None else gl.attention_map()
            gemm(G, h, transA=True, out=self.dW_s[l])
            dT = spmm_reduce_bwd(gl.rowptr_t, gl.colidx_t, map_t, arg, G, out=self._tmp(("dT", l), (n, self.dims[l + 1])))
            gemm(dT, h, transA=True, out=self.dW_n[l])
            if l == 0 and not input_grad:
                return None
            dh = gemm(G, self.W_s[l], out=self._tmp(("dh", l), (n, self.dims[l])))     # through the vertex itself
            gemm(dT, self.W_n[l], out=dh, beta=1.0)                                    # + through its neighbourhood
            if l == 0:
                return dh
            G = relu_mask(h, dh, out=self._tmp(("G", l), (n, self.dims[l])))           # h = relu output of the layer below
            colsum(G, out=self.db[l - 1])
        return G


# ---- graph readout: segment pooling, graph batches, a classifier head (include/gnnx.h "graph readout") ----------------------------------
POOL_OPS = {"sum": 0, "mean": 1, "max": 2}   # GNNX_POOL_SUM / GNNX_POOL_MEAN / GNNX_POOL_MAX
POOL_CHUNK = 256                             # GNNX_POOL_CHUNK


def _pool_sizes(segptr, where):
    if segptr.dtype != torch.int32 or segptr.dim() != 1 or not segptr.is_contiguous() or segptr.numel() < 1:
        raise capi.GnnxError(-2, where, "segptr must be a contiguous int32 vector of n_seg + 1 entries")
    return int(segptr.numel()) - 1


def _pool_matrix(t, shape, dtype, what, where):
    """t must be a 2-D `dtype` matrix of `shape` (None: any) whose rows are contiguous: its pointer and row stride go to the kernel as
    they are."""
    if t.dim() != 2 or t.dtype != dtype or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "" if shape is None else f" {tuple(shape)}"
        raise capi.GnnxError(-2, where, f"{what} must be a 2-D {dtype} matrix{want} with unit inner stride, got {t.dtype} "
                                        f"{tuple(t.shape)} strides {tuple(t.stride())}")
    return t


def segment_pool(segptr, X, op="sum", out=None, arg_out=None, want_arg=True):
    """gnnx_segment_pool_f32: (Y, arg) with Y[b] the sum / mean / max of the rows [segptr[b], segptr[b+1]) of X and, for op="max" with
    want_arg, arg[b, f] = the first row of the segment that attains the maximum (int32, an absolute row of X; -1 for an empty segment);
    arg is None otherwise.  An empty segment gives +0.  The sum has the order of include/gnnx.h "graph readout": a segment's bits depend on
    its own rows alone.  X, out and arg_out may be strided views."""
    if op not in POOL_OPS:
        raise capi.GnnxError(-1, "segment_pool", f"op must be 'sum', 'mean' or 'max', got {op!r}")
    n_seg = _pool_sizes(segptr, "segment_pool")
    n_rows, F = _pool_matrix(X, None, torch.float32, "X", "segment_pool").shape
    if out is None:
        out = torch.empty((n_seg, F), dtype=torch.float32, device=X.device)
    arg = None
    if op == "max" and want_arg:
        arg = torch.empty((n_seg, F), dtype=torch.int32, device=X.device) if arg_out is None else arg_out
        _pool_matrix(arg, (n_seg, F), torch.int32, "arg_out", "segment_pool")
    _pool_matrix(out, (n_seg, F), torch.float32, "out", "segment_pool")
    ws, wsb = _scratch("gnnx_segment_pool_workspace", n_seg, n_rows, F, device=X.device, tag="pool")
    capi.call("gnnx_segment_pool_f32", POOL_OPS[op], n_seg, n_rows, F, _ptr(segptr), _ptr(X) if X.numel() else None, _ld(X), _ptr(out), _ld(out),
              _ptr(arg), _ld(arg) if arg is not None else 0, _ptr(ws), wsb, _stream())
    return out, arg


def segment_pool_bwd(segptr, G, op, arg=None, out=None, beta=0.0, n_rows=None):
    """gnnx_segment_pool_bwd_f32: dX = beta * dX + the gradient of segment_pool with respect to X: row i of segment b receives G[b] (sum),
    G[b] / len (mean) or G[b, f] where arg[b, f] == i (max; arg from the forward).  Every row of dX is written; beta = 0 never reads it.
    n_rows (an addition to the call's documented arguments, only read without `out`): the rows of the dX to allocate; without it they
    are segptr's last entry, which costs a device read and a synchronisation."""
    if op not in POOL_OPS:
        raise capi.GnnxError(-1, "segment_pool_bwd", f"op must be 'sum', 'mean' or 'max', got {op!r}")
    n_seg = _pool_sizes(segptr, "segment_pool_bwd")
    if G.dim() != 2 or int(G.shape[0]) != n_seg:
        raise capi.GnnxError(-2, "segment_pool_bwd", f"G must be [{n_seg}, F], got {tuple(G.shape)}")
    F = int(_pool_matrix(G, None, torch.float32, "G", "segment_pool_bwd").shape[1])
    if op == "max":
        if arg is None:
            raise capi.GnnxError(-2, "segment_pool_bwd", f"op 'max' needs the forward's int32 arg {(n_seg, F)}")
        _pool_matrix(arg, (n_seg, F), torch.int32, "arg", "segment_pool_bwd")
    if out is None:
        if beta != 0.0:
            raise capi.GnnxError(-1, "segment_pool_bwd", "beta = 1 needs the matrix to add to (out)")
        if n_rows is None:
            n_rows = int(segptr[-1])
        out = torch.empty((n_rows, F), dtype=torch.float32, device=G.device)
    _pool_matrix(out, None, torch.float32, "out", "segment_pool_bwd")
    n_rows = int(out.shape[0])
    if int(out.shape[1]) != F:
        raise capi.GnnxError(-2, "segment_pool_bwd", f"out must be [n_rows, {F}], got {tuple(out.shape)}")
    use_arg = arg if op == "max" else None
    capi.call("gnnx_segment_pool_bwd_f32", POOL_OPS[op], n_seg, n_rows, F, _ptr(segptr), _ptr(use_arg), _ld(use_arg) if use_arg is not None else 0,
              _ptr(G), _ld(G), float(beta), _ptr(out) if out.numel() else None, _ld(out), _stream())
    return out


# ---- nearest neighbours (include/gnnx.h "nearest neighbours") ----------------------------------------------------------------------------
KNN_MAX_K = 64                                # GNNX_KNN_MAX_K
KNN_EXCLUDE_SELF, KNN_NEAREST_FIRST = 1, 2    # GNNX_KNN_EXCLUDE_SELF / GNNX_KNN_NEAREST_FIRST


def _row_pitch(t):
    """Row stride of a 2-D matrix for the C-ABI; a matrix of at most one row has none worth the name."""
    return t.stride(0) if int(t.shape[0]) > 1 else max(int(t.shape[1]), 1)


def knn(X, k, Q=None, segptr=None, qsegptr=None, exclude_self=False, nearest_first=False, want_dist=True):
    """gnnx_knn_f32: (idx int32 [m, k], dist float32 [m, k] or None).  Row i of idx holds the rows of X nearest to query i -- a row of Q,
    or of X itself without Q -- among the candidates of its own segment (segptr / qsegptr: int32 [n_seg + 1], e.g. a GraphBatch's
    graph_ptr; neither: one segment), by squared Euclidean distance with ties to the smaller row and NaN last; -1 (dist: +inf) where
    the segment has fewer than k candidates.  exclude_self drops the candidate with the query's own row number (meant for Q=None).
    The kept entries stand in ascending ROW order (a strictly ascending CSR row), with nearest_first in ascending distance order.
    X and Q may be strided views.  The result is a function of the inputs alone, bit for bit."""
    k = int(k)
    n, F = _pool_matrix(X, None, torch.float32, "X", "knn").shape
    m = n if Q is None else int(_pool_matrix(Q, None, torch.float32, "Q", "knn").shape[0])
    if Q is not None and int(Q.shape[1]) != F:
        raise capi.GnnxError(-2, "knn", f"Q has {int(Q.shape[1])} columns, X has {F}")
    n_seg = 1 if segptr is None else _pool_sizes(segptr, "knn")
    if Q is not None and (segptr is None) != (qsegptr is None):
        raise capi.GnnxError(-2, "knn", "segptr and qsegptr come together")
    if Q is not None and qsegptr is not None and _pool_sizes(qsegptr, "knn") != n_seg:
        raise capi.GnnxError(-2, "knn", f"qsegptr must have {n_seg + 1} entries like segptr")
    idx = torch.empty((m, max(k, 0)), dtype=torch.int32, device=X.device)
    dist = torch.empty((m, max(k, 0)), dtype=torch.float32, device=X.device) if want_dist else None
    if Q is not None and m == 0:
        return idx, dist
    flags = (KNN_EXCLUDE_SELF if exclude_self else 0) | (KNN_NEAREST_FIRST if nearest_first else 0)
    capi.call("gnnx_knn_f32", n, m, F, n_seg, _ptr(X) if n else None, _row_pitch(X), _ptr(segptr), _ptr(Q), 0 if Q is None else _row_pitch(Q),
              _ptr(qsegptr) if Q is not None else None, k, flags, _ptr(idx) if m else None, max(k, 1), _ptr(dist) if m else None, max(k, 1),
              _stream())
    return idx, dist


def knn_graph(X, k, graph_ptr=None, loop=False, transpose=True, norm=True):
    """The k-nearest-neighbour graph of the rows of X (knn with exclude_self = not loop): row i stores its k nearest rows, ascending, so
    messages flow from neighbour to vertex (SageStack's convention).  graph_ptr (int32 [B + 1]): X holds B clouds, cloud b the rows
    graph_ptr[b] .. graph_ptr[b + 1] - 1, no edge joins two clouds and the result is a GraphBatch; without it a CsrGraph.  A cloud of
    k points or fewer gives short rows, a cloud of one point an empty row.  The CSR is the flattened idx (short rows masked out); the
    transposed CSR is built from the COO (column, row) with self loops and duplicates kept -- exactly the transposed entries.  Plans
    are not made."""
    n, dev = int(X.shape[0]), X.device
    if graph_ptr is not None:
        graph_ptr = torch.as_tensor(graph_ptr).to(device=dev, dtype=torch.int32).contiguous()
    idx, _ = knn(X, k, segptr=graph_ptr, exclude_self=not loop, want_dist=False)
    k = int(k)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    if n == 0 or int(idx[:, k - 1].min()) >= 0:        # no row is short
        rowptr = torch.arange(n + 1, dtype=torch.int32, device=dev) * k
        colidx, rowid = idx.reshape(-1), rows.repeat_interleave(k)
    else:
        keep = idx >= 0
        rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        rowptr[1:] = torch.cumsum(keep.sum(1), 0).to(torch.int32)
        colidx, rowid = idx[keep].contiguous(), rows.repeat_interleave(keep.sum(1))
    if graph_ptr is None:
        g = CsrGraph(n, rowptr, colidx)
    else:
        g = GraphBatch(n, rowptr, colidx)
        g.graph_ptr, g.n_graphs = graph_ptr, int(graph_ptr.numel()) - 1
    if transpose:
        if g.nnz:
            g.rowptr_t, g.colidx_t = CsrGraph.csr_from_coo(colidx, rowid, n, flags=3)   # keep self loops and duplicates
        else:
            g.rowptr_t, g.colidx_t = torch.zeros_like(rowptr), colidx.clone()
    if norm:
        g.compute_norm()
    return g


class GraphBatch(CsrGraph):
    """A batch of B small graphs as ONE block-diagonal CsrGraph that every stack takes unchanged: graph k owns the consecutive vertices
    graph_ptr[k] .. graph_ptr[k+1] - 1 and no edge joins two graphs.  graph_ptr: device int32 [B + 1] (segment_pool's segptr); n_graphs;
    batch: int32 [n], the graph of each vertex (built when first asked for).  There is no relabelling: it would break the contiguity of
    a graph's vertices that the readout rests on."""

    graph_ptr = None
    n_graphs = 0
    _batch = None

    @classmethod
    def from_graphs(cls, graphs, transpose=True, norm=True):
        """graphs: [(src, dst, n_i), ...] with device int32 edge lists on the graph's own vertex ids 0 .. n_i - 1."""
        if not graphs:
            raise ValueError("a batch needs at least one graph")
        ptr = [0]
        for _, _, n_i in graphs:
            if int(n_i) < 0:
                raise ValueError("negative vertex count")
            ptr.append(ptr[-1] + int(n_i))
        if ptr[-1] >= 2 ** 31:
            raise ValueError("the batch does not fit int32 vertex ids")
        src = torch.cat([s.to(torch.int32) + off for (s, _, _), off in zip(graphs, ptr)])
        dst = torch.cat([d.to(torch.int32) + off for (_, d, _), off in zip(graphs, ptr)])
        # ONE check of the concatenated list: both endpoints of every edge lie in the vertex range of the graph that listed the edge
        dev = src.device
        graph_ptr = torch.tensor(ptr, dtype=torch.int64, device=dev)
        owner = torch.repeat_interleave(torch.arange(len(graphs), device=dev), torch.tensor([int(s.numel()) for s, _, _ in graphs], device=dev))
        lo, hi = graph_ptr[owner], graph_ptr[owner + 1]
        if src.numel() != dst.numel() or bool(((src < lo) | (src >= hi) | (dst < lo) | (dst >= hi)).any()):
            raise ValueError("an edge names a vertex outside its graph")
        return cls._build(src, dst, graph_ptr.to(torch.int32), ptr[-1], transpose, norm)

    @classmethod
    def from_coo_batched(cls, src, dst, graph_ptr, transpose=True, norm=True):
        """An already concatenated edge list on the batch's vertex ids.  ValueError if graph_ptr is not non-decreasing from 0, if an edge
        names a vertex outside the batch or if an edge joins two graphs."""
        ptr = torch.as_tensor(graph_ptr).to(torch.int64).cpu().reshape(-1)
        if ptr.numel() < 2 or int(ptr[0]) != 0 or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError("graph_ptr must be non-decreasing from 0, with one entry more than there are graphs")
        n = int(ptr[-1])
        if n >= 2 ** 31:
            raise ValueError("the batch does not fit int32 vertex ids")
        if src.numel():
            if int(min(src.min(), dst.min())) < 0 or int(max(src.max(), dst.max())) >= n:
                raise ValueError("an edge names a vertex outside the batch")
            ends = ptr[1:].to(src.device)
            if bool((torch.bucketize(src.long(), ends, right=True) != torch.bucketize(dst.long(), ends, right=True)).any()):
                raise ValueError("an edge joins two graphs of the batch")
        return cls._build(src.to(torch.int32), dst.to(torch.int32), ptr.to(torch.int32).to(src.device), n, transpose, norm)

    @classmethod
    def _build(cls, src, dst, graph_ptr, n, transpose, norm):
        g = cls.from_coo(src, dst, n, transpose=transpose, norm=norm, relabel=None)
        g.graph_ptr = graph_ptr.contiguous()
        g.n_graphs = int(graph_ptr.numel()) - 1
        return g

    @classmethod
    def of_points(cls, graph_ptr, device=None):
        """An EDGELESS batch whose rows are owned as graph_ptr says: what a stack that builds its own graphs (EdgeConvStack with k) and
        GraphClassifier bind to when the data is B point clouds.  Both CSRs are empty; s / norm are not made."""
        ptr = torch.as_tensor(graph_ptr)
        dev = device if device is not None else (ptr.device if ptr.is_cuda else "cuda")
        host = ptr.to(torch.int64).cpu().reshape(-1)
        if host.numel() < 2 or int(host[0]) != 0 or bool((host[1:] < host[:-1]).any()):
            raise ValueError("graph_ptr must be non-decreasing from 0, with one entry more than there are graphs")
        n = int(host[-1])
        if n >= 2 ** 31:
            raise ValueError("the batch does not fit int32 vertex ids")
        rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        colidx = torch.empty(0, dtype=torch.int32, device=dev)
        g = cls(n, rowptr, colidx, rowptr.clone(), colidx.clone())
        g.graph_ptr = host.to(torch.int32).to(dev).contiguous()
        g.n_graphs = int(host.numel()) - 1
        return g

    @property
    def batch(self):
        if self._batch is None:
            counts = (self.graph_ptr[1:] - self.graph_ptr[:-1]).long()
            ids = torch.arange(self.n_graphs, dtype=torch.int32, device=self.graph_ptr.device)
            self._batch = torch.repeat_interleave(ids, counts)
        return self._batch


class GraphClassifier(_Model):
    """One answer per GRAPH of a GraphBatch: a readout and a linear head over any of the three stacks,
        Z = segment_pool(net.forward(X), pool) [B, dims[-1]];   logits = Z W_c^T + b_c   [B, n_classes],
    trained through the readout.  forward / backward / step / train_step / evaluate (no row selection: every graph of the batch counts),
    and on_batch for an epoch over mini-batches of any size.  Every operation is a C-ABI call: the stack's own, segment_pool, gemm,
    bias_add, softmax_ce (db_c from the loss kernel), segment_pool_bwd into net.grad_buffer(), sgd_step.  No atomics on any value; the
    same bits every run.

    The stack is bound to the batch with net._view()._bind(batch), for any vertex count: a stack of the same class on the same parameter
    and gradient tensors, with what its _bind derives from the batch and scratch buffers of its own (they are shaped by the vertex count)."""

    def __init__(self, net, batch, n_classes, pool="mean", seed=0):
        if pool not in POOL_OPS:
            raise ValueError(f"pool must be 'sum', 'mean' or 'max', got {pool!r}")
        if not isinstance(batch, GraphBatch):
            raise TypeError("batch must be a GraphBatch")
        if not isinstance(net, _Stack):
            raise TypeError(f"GcnStack, GatStack or SageStack expected, got {type(net).__name__}")
        self.net = net if net.g is batch else net._view()._bind(batch)
        self.batch, self.pool, self.n_classes = batch, pool, int(n_classes)
        d = self.net.dims[-1]
        dev = batch.graph_ptr.device
        self.W_c = uniform_pm1(seed + 1000, (self.n_classes, d), scale=d ** -0.5, device=dev)
        self.b_c = torch.zeros(self.n_classes, dtype=torch.float32, device=dev)
        self.dW_c = torch.zeros_like(self.W_c)
        self.db_c = torch.zeros_like(self.b_c)
        self._saved = None
        self._buf = {}
        self._opt = [None]

    def on_batch(self, batch):
        """This classifier on another GraphBatch, of ANY vertex and graph count: it shares W_c, b_c, their gradients and the stack's
        parameters and gradients (the same tensors), and binds the stack to the new graph:
            for b in batches: clf.on_batch(b).train_step(X_b, target_b, lr)"""
        if not isinstance(batch, GraphBatch):
            raise TypeError("batch must be a GraphBatch")
        return self._view(net=self.net._view()._bind(batch), batch=batch)

    def params(self):
        return self.net.params() + [self.W_c, self.b_c]

    def grads(self):
        return self.net.grads() + [self.dW_c, self.db_c]

    def forward(self, X):
        """logits [B, n_classes]; the pooled Z [B, dims[-1]] is kept (self.Z) with the readout's arg for backward."""
        B, d = self.batch.n_graphs, self.net.dims[-1]
        H = self.net.forward(X)
        Z, arg = segment_pool(self.batch.graph_ptr, H, self.pool, out=self._tmp("Z", (B, d)),
                              arg_out=self._tmp("arg", (B, d), torch.int32) if self.pool == "max" else None)
        logits = bias_add(gemm(Z, self.W_c, transB=True, out=self._tmp("ZW", (B, self.n_classes))), self.b_c, out=self._tmp("logits", (B, self.n_classes)))
        self._saved = (Z, arg)
        self.Z = Z
        return logits

    def backward(self, dlogits, have_bias_grad=False):
        """dW_c, db_c and every gradient of the stack from dlogits = dL/dlogits.  have_bias_grad: db_c was already written by the loss
        kernel (softmax_ce(..., colsum_out=clf.db_c))."""
        Z, arg = self._saved
        if not have_bias_grad:
            colsum(dlogits, out=self.db_c)
        gemm(dlogits, Z, transA=True, out=self.dW_c)
        dZ = gemm(dlogits, self.W_c, out=self._tmp("dZ", tuple(Z.shape)))
        dH = segment_pool_bwd(self.batch.graph_ptr, dZ, self.pool, arg=arg, out=self.net.grad_buffer())
        self.net.backward(dH, input_grad=False)

    def train_step(self, X, target, lr, weight_decay=0.0):
        """One step of the model's optimiser (plain SGD by default) on the batch: forward -> softmax_ce over the B graphs (db_c from the
        loss kernel) -> backward through the readout and the stack, no input gradient -> step.  target: int32 [B].  Returns the
        loss tensor."""
        logits = self.forward(X)
        loss, d = softmax_ce(logits, target, colsum_out=self.db_c, grad_out=self._tmp("dlogits", tuple(logits.shape)))
        self.backward(d, have_bias_grad=True)
        self.step(lr, weight_decay)
        return loss

    def evaluate(self, X, target):
        """(loss as a 1-element tensor, correctly classified graphs, B)."""
        logits = self.forward(X)
        return (softmax_ce(logits, target, want_grad=False)[0], *accuracy(logits, target))
