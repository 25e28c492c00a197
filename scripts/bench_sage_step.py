#!/usr/bin/env python3
"""Measurement (GPU box): the neighbourhood reductions of a GraphSAGE max layer -- ops.spmm_reduce (max, with its arg) and
ops.spmm_reduce_bwd -- and one SageStack.train_step per aggregator, with the PLANNED ops.spmm on CSR(A) and on CSR(A^T) at the same
width in the same process as the yardsticks (each gathers nnz * 4 F bytes of rows; the reduce forward gathers the same and writes
8 F bytes per row, value and arg; the reduce backward gathers nnz * 8 F, the arg row and the G row: DESIGN.md section 5.4).

    every kernel: --repeats single calls between two device events after --warmup calls; the median and the range are reported

One JSON line per configuration:

    rmat1m    R-MAT 1 M vertices / 10 M edges, F = 128, plus one training step of SageStack([128, 128, 128]) for each aggregator over a
              tenth of the rows
    headline  R-MAT 10 M vertices / 100 M edges, F = 256 (BASELINE.md's headline graph), kernels only

The graph is NOT relabelled (the max layer's transpose map needs ascending rows), so the aggregation yardstick here is not BASELINE.md's
scrambled-order number.  Without --config the script is a driver: it runs every configuration as a child process of its own under a
time limit and stops at the first one that fails.
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

CONFIGS = {"rmat1m": dict(nodes=1_000_000, edges=10_000_000, feat=128, step=True, limit=300),
           "headline": dict(nodes=10_000_000, edges=100_000_000, feat=256, step=False, limit=420)}


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
    n, e, F = cfg["nodes"], cfg["edges"], cfg["feat"]

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

    src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(src, dst, n)
    g.make_plans(args.chunk, F)
    map_t = g.attention_map()
    deg, deg_t = g.rowptr[1:] - g.rowptr[:-1], g.rowptr_t[1:] - g.rowptr_t[:-1]
    X = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    G = ops.uniform_pm1(args.seed + 2, (n, F), device=dev)
    Y = torch.empty((n, F), dtype=torch.float32, device=dev)
    arg = torch.empty((n, F), dtype=torch.int32, device=dev)
    dX = torch.empty((n, F), dtype=torch.float32, device=dev)
    ops.spmm_reduce(g.rowptr, g.colidx, X, out=Y, arg_out=arg)
    kernels = {
        "spmm_planned": lambda: ops.spmm(g.rowptr, g.colidx, X, out=Y, plan=g.plan),
        "spmm_planned_t": lambda: ops.spmm(g.rowptr_t, g.colidx_t, G, out=dX, plan=g.plan_t),
        "spmm_reduce_max": lambda: ops.spmm_reduce(g.rowptr, g.colidx, X, out=Y, arg_out=arg),
        "spmm_reduce_bwd": lambda: ops.spmm_reduce_bwd(g.rowptr_t, g.colidx_t, map_t, arg, G, out=dX),
    }
    order = ("spmm_reduce_max", "spmm_reduce_bwd", "spmm_planned", "spmm_planned_t")   # the yardsticks overwrite Y last: arg stays the forward's
    ms = {k: timed(kernels[k]) for k in order}
    med = {k: statistics.median(v) for k, v in ms.items()}
    model_fwd = g.nnz * (4 * F + 4) + n * (8 * F + 4)             # gathered rows + colidx; value and arg per row + rowptr
    model_bwd = g.nnz * (8 * F + 8) + n * (4 * F + 4)             # gathered G and arg rows + colidx_t, map_t; dX per row
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "feat": F, "chunk": args.chunk,
           "max_degree": int(deg.max()), "max_degree_share_of_nnz": round(int(deg.max()) / max(g.nnz, 1), 6),
           "max_degree_t": int(deg_t.max()), "max_degree_t_share_of_nnz": round(int(deg_t.max()) / max(g.nnz, 1), 6),
           "rows_over_4096": int((deg > 4096).sum()), "rows_t_over_4096": int((deg_t > 4096).sum()),
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "spmm_reduce_max_model_TBps": round(model_fwd / med["spmm_reduce_max"] / 1e9, 3),
           "spmm_reduce_bwd_model_TBps": round(model_bwd / med["spmm_reduce_bwd"] / 1e9, 3),
           "spmm_planned_model_TBps": round((g.nnz * (4 * F + 4) + n * (4 * F + 4)) / med["spmm_planned"] / 1e9, 3),
           "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
    if cfg["step"]:
        del Y, dX, arg, G
        Xs = X
        target = (torch.arange(n, device=dev) % F).to(torch.int32)
        rows = torch.arange(0, n, 10, device=dev, dtype=torch.int32)
        out["sage_dims"] = [F, F, F]
        for aggr in ("mean", "max"):
            net = ops.SageStack(g, [F, F, F], aggr=aggr, seed=args.seed + 100, device=dev)
            t = timed(lambda: net.train_step(Xs, target, rows, 0.0))
            out[f"train_step_{aggr}_ms"] = [round(x, 4) for x in t]
            out[f"train_step_{aggr}_ms_median"] = round(statistics.median(t), 4)
            del net
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default="rmat1m,headline", help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
