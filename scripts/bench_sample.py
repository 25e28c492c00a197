#!/usr/bin/env python3
"""Measurement (GPU box): the neighbour sampler, ops.sample_neighbors (gnnx_csr_sample_neighbors), at k = 10 and 25.

    every figure: --repeats single calls after --warmup calls under a host clock (the sampler synchronises its stream; the other legs
    are followed by a device synchronisation inside the clock); the median and the range are reported

Beside the sampler, in the same process:
    copy       a device copy of rowptr + colidx: the floor of any pass over the pattern
    uniform    the same call on a graph of the same n and as many generated edges with uniform endpoints (R-MAT with a = b = c = 1/4):
               no hub rows; the difference to the R-MAT time is what the hubs cost
    longest    the same call on a one-row CSR that holds the R-MAT graph's longest row alone: the segment + combine path (the long-row
               kernel at 257 .. 4096 entries) with nothing to hide behind
and with --config rmat1m one training epoch as a user runs it, SageStack([128, 128, 128]) over a tenth of the rows for each aggregator:
train_step on the full graph against g.sample_neighbors(10, seed) + net.on_graph(...).train_step.

One JSON line per configuration:
    rmat1m    R-MAT 1 M vertices / 10 M edges
    headline  R-MAT 10 M vertices / 100 M edges (BASELINE.md's headline graph), sampler only

Without --config the script is a driver: it runs every configuration as a child process of its own under a time limit and stops at
the first one that fails.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"rmat1m": dict(nodes=1_000_000, edges=10_000_000, step=True, limit=300),
           "headline": dict(nodes=10_000_000, edges=100_000_000, step=False, limit=420)}
FANOUTS = (10, 25)


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
    n, e = cfg["nodes"], cfg["edges"]

    def timed(fn):
        def once():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(args.warmup):
            once()
        return [once() for _ in range(args.repeats)]

    def stats(ms):
        return {"ms_median": round(statistics.median(ms), 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)]}

    def graph(a, b, c, transpose):
        src, dst = ops.rmat_edges(args.seed, n, e, a, b, c, device=dev)
        return ops.CsrGraph.from_coo(src, dst, n, transpose=transpose, norm=False)

    def sampler(rowptr, colidx, k):
        kept = []
        ms = timed(lambda: kept.append(int(ops.sample_neighbors(rowptr, colidx, k, args.seed, want_rowid=True)[1].numel())))
        return dict(stats(ms), kept=kept[-1])

    g = graph(0.57, 0.19, 0.19, cfg["step"])
    deg = g.rowptr[1:] - g.rowptr[:-1]
    longest = int(deg.argmax())
    b, d = int(g.rowptr[longest]), int(deg[longest])
    one_row = torch.tensor([0, d], dtype=torch.int32, device=dev)
    copy_r, copy_c = torch.empty_like(g.rowptr), torch.empty_like(g.colidx)
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "max_degree": d, "rows_over_4096": int((deg > 4096).sum()),
           "entries_in_rows_over_4096": int(deg[deg > 4096].sum()),
           "copy": stats(timed(lambda: (copy_r.copy_(g.rowptr), copy_c.copy_(g.colidx)))), "repeats": args.repeats, "warmup": args.warmup,
           "device": capi.device_name(0)}
    for k in FANOUTS:
        out[f"rmat_k{k}"] = sampler(g.rowptr, g.colidx, k)
        out[f"longest_row_k{k}"] = sampler(one_row, g.colidx[b:b + d].clone(), k)
    u = graph(0.25, 0.25, 0.25, False)
    out["uniform_nnz"], out["uniform_max_degree"] = u.nnz, int((u.rowptr[1:] - u.rowptr[:-1]).max())
    for k in FANOUTS:
        out[f"uniform_k{k}"] = sampler(u.rowptr, u.colidx, k)
    del u, copy_r, copy_c
    if cfg["step"]:
        F, k = 128, 10
        g.compute_norm()
        g.make_plans(args.chunk, F)
        X = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
        target = (torch.arange(n, device=dev) % F).to(torch.int32)
        rows = torch.arange(0, n, 10, device=dev, dtype=torch.int32)
        out["sage_dims"], out["epoch_fanout"] = [F, F, F], k
        seeds = iter(range(10 ** 6))      # a fresh seed per epoch
        out["sampled_graph"] = stats(timed(lambda: g.sample_neighbors(k, next(seeds))))   # sample + transposed CSR + norm + plans
        for aggr in ("mean", "max"):
            net = ops.SageStack(g, [F, F, F], aggr=aggr, seed=args.seed + 100, device=dev)
            out[f"epoch_full_{aggr}"] = stats(timed(lambda: net.train_step(X, target, rows, 0.0)))
            out[f"epoch_sampled_{aggr}"] = stats(timed(lambda: net.on_graph(g.sample_neighbors(k, next(seeds))).train_step(X, target, rows, 0.0)))
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
