#!/usr/bin/env python3
"""Measurement (GPU box): the edge-feature aggregation of a GINE layer -- ops.spmm_edge (ReLU message) and its backward, ops.spmm_edge_bwd
plus the dX call on CSR(A^T) -- against the torch composition a caller had to write before (index, add, clamp, index_add_: three
[nnz, F] round trips and atomics) and against plain ops.spmm on the same pattern as the floor (it reads no E), in one process.

    every kernel: --repeats single calls between two device events after --warmup calls; the median and the range are reported

Byte model, per call, against the 8 TB/s HBM specification (every matrix counted once, although X / G rows are gathered from cache):
    spmm_edge      nnz * (4 F [E row] + 4 F [X row] + 4 [colidx])  + n * (4 F [Y] + 4 [rowptr])          (+ 4 nnz with eidx)
    spmm_edge_bwd  nnz * (4 F [E] + 4 F [X] + 4 F [dE store] + 4)  + n * (4 F [G] + 4)                   (+ 4 nnz with eidx)
    dX             nnz * (4 F [dE row] + 8 [colidx_t, eidx_t])     + n * (8 F [dX read and written] + 4)
    spmm (floor)   nnz * (4 F + 4) + n * (4 F + 4)

One JSON line per configuration:

    rmat1m_f64 / rmat1m_f128   R-MAT 1 M vertices / 10 M edges, one attribute row per stored entry
    batch4096                  4096 graphs of 25 vertices and 60 listed edges each as one GraphBatch, F = 64, plus one
                               GraphClassifier(GineStack([64, 64, 64], edge_dim 8)).train_step

With GNNX_HIP_LIB=exp (the measurement build) the E stream without eidx is timed both ways, GNNX_EDGE_E_LOAD=nt / plain.  Without
--config the script is a driver: it runs every configuration as a child process of its own under a time limit and stops at the first
one that fails.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"rmat1m_f64": dict(nodes=1_000_000, edges=10_000_000, feat=64, limit=300),
           "rmat1m_f128": dict(nodes=1_000_000, edges=10_000_000, feat=128, limit=300),
           "batch4096": dict(graphs=4096, nodes_each=25, edges_each=60, feat=64, limit=300)}
HBM_SPEC_TBPS = 8.0


def driver(args):
    for name in args.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, timeout=CONFIGS[name]["limit"])
        except subprocess.TimeoutExpired:
            print(json.dumps({"config": name, "error": "time limit"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"config": name, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


def measure(args):
    import torch

    from __graft_entry__ import load_package
    load_package()
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    F = cfg["feat"]

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def one_call_ms(fn):
        a, b = capi.Event(), capi.Event()
        a.record(stream())
        fn()
        b.record(stream())
        b.sync()
        return a.elapsed_ms(b)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return [one_call_ms(fn) for _ in range(args.repeats)]

    if "graphs" in cfg:
        B, nv, ne = cfg["graphs"], cfg["nodes_each"], cfg["edges_each"]
        n = B * nv
        off = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(ne) * nv
        torch.manual_seed(args.seed)
        s, d = (torch.randint(0, nv, (B * ne,), device=dev, dtype=torch.int32) for _ in range(2))   # uniform endpoints inside each graph
        src, dst = s + off, d + off
        g = ops.GraphBatch.from_coo_batched(src, dst, torch.arange(B + 1, dtype=torch.int32) * nv)
    else:
        n = cfg["nodes"]
        src, dst = ops.rmat_edges(args.seed, n, cfg["edges"], 0.57, 0.19, 0.19, device=dev)
        g = ops.CsrGraph.from_coo(src, dst, n)
    nnz = g.nnz
    map_t = g.attention_map()
    perm = torch.randperm(nnz, device=dev).to(torch.int32)                               # attribute rows in a caller's order
    perm_t = perm[map_t.long()].contiguous()
    X = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    E = ops.uniform_pm1(args.seed + 2, (nnz, F), device=dev)
    G = ops.uniform_pm1(args.seed + 3, (n, F), device=dev)
    Y, dX, dE = torch.empty_like(X), torch.empty_like(X), torch.zeros_like(E)
    rows_l = torch.repeat_interleave(torch.arange(n, device=dev), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols_l, perm_l = g.colidx.long(), perm.long()

    def torch_fwd():
        m = (X[cols_l] + E[perm_l]).clamp_(min=0)
        return Y.zero_().index_add_(0, rows_l, m)

    def torch_bwd():
        dm = G[rows_l] * ((X[cols_l] + E[perm_l]) > 0)
        dE[perm_l] = dm
        return dX.zero_().index_add_(0, cols_l, dm)

    def edge_bwd(eidx, eidx_t):
        ops.spmm_edge_bwd(g.rowptr, g.colidx, X, E, G, eidx=eidx, out=dE)
        dX.zero_()
        return ops.spmm_edge(g.rowptr_t, g.colidx_t, None, dE, eidx=eidx_t, msg="add", out=dX, beta=1.0, n_cols=n)

    kernels = {
        "spmm_edge_stream": lambda: ops.spmm_edge(g.rowptr, g.colidx, X, E, out=Y),
        "spmm_edge_eidx": lambda: ops.spmm_edge(g.rowptr, g.colidx, X, E, eidx=perm, out=Y),
        "edge_bwd_stream": lambda: edge_bwd(None, map_t),
        "edge_bwd_eidx": lambda: edge_bwd(perm, perm_t),
        "torch_fwd": torch_fwd, "torch_bwd": torch_bwd,
        "spmm_floor": lambda: ops.spmm(g.rowptr, g.colidx, X, out=Y),
        "spmm_floor_t": lambda: ops.spmm(g.rowptr_t, g.colidx_t, G, out=dX),
    }
    ms = {k: timed(fn) for k, fn in kernels.items()}
    if os.environ.get("GNNX_HIP_LIB") == "exp":
        for how in ("nt", "plain") * 3:                                   # alternating, so that drift hits both alike
            os.environ["GNNX_EDGE_E_LOAD"] = how
            ms.setdefault("spmm_edge_stream_" + how, []).extend(timed(kernels["spmm_edge_stream"]))
        del os.environ["GNNX_EDGE_E_LOAD"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    model = {"spmm_edge_stream": nnz * (8 * F + 4) + n * (4 * F + 4), "spmm_edge_eidx": nnz * (8 * F + 8) + n * (4 * F + 4),
             "edge_bwd_stream": nnz * (12 * F + 4) + n * (4 * F + 4) + nnz * (4 * F + 8) + n * (8 * F + 4),
             "edge_bwd_eidx": nnz * (12 * F + 8) + n * (4 * F + 4) + nnz * (4 * F + 8) + n * (8 * F + 4),
             "spmm_floor": nnz * (4 * F + 4) + n * (4 * F + 4)}
    deg = g.rowptr[1:] - g.rowptr[:-1]
    out = {"config": args.config, "nodes": n, "nnz": nnz, "feat": F, "max_degree": int(deg.max()), "rows_over_4096": int((deg > 4096).sum()),
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "model_TBps": {k: round(b / med[k] / 1e9, 3) for k, b in model.items()},
           "share_of_hbm_spec": {k: round(b / med[k] / 1e9 / HBM_SPEC_TBPS, 3) for k, b in model.items()},
           "repeats": args.repeats, "warmup": args.warmup, "library": os.environ.get("GNNX_HIP_LIB", "product"), "device": capi.device_name(0)}
    if "graphs" in cfg:
        g.set_edge_attr(src, dst, ops.uniform_pm1(args.seed + 4, (int(src.numel()), 8), device=dev))
        clf = ops.GraphClassifier(ops.GineStack(g, [F, F, F], 8, seed=args.seed + 100, device=dev), g, 8)
        target = (torch.arange(g.n_graphs, device=dev) % 8).to(torch.int32)
        t = timed(lambda: clf.train_step(X, target, 0.0))
        out["classifier_train_step_ms"], out["classifier_train_step_ms_median"] = [round(x, 4) for x in t], round(statistics.median(t), 4)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default=",".join(CONFIGS), help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
