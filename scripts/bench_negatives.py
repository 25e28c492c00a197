#!/usr/bin/env python3
"""Measurement (GPU box): negative sampling off the graph, CsrGraph.sample_negatives (gnnx_csr_sample_negatives),
at m = 1 and m = 5 negatives per positive, and one link-prediction epoch with fresh negatives.

    every figure: --repeats single calls after --warmup calls under a host clock (the sampler synchronises its stream; the other legs
    are followed by a device synchronisation inside the clock); the median and the range are reported

Beside each figure, in the same process, the recipe that EdgeSet.from_pairs' docstring gave before: as many uniform pairs from
rmat_edges(seed, n, k, a=.25, b=.25, c=.25), listed before the positives.
    sampler_m*       g.sample_negatives(m, seed): nnz * m draws from the non-edges
    recipe_draw_m*   rmat_edges of nnz * m uniform pairs
    recipe_share_m*  the share of those pairs that are true edges or self pairs (counted once, by a search of the pair keys in the
                     graph's sorted keys)
    copy             a device copy of rowptr + colidx: the floor of any pass over the pattern
    edge_set_graph   EdgeSet.from_graph(g, 1, seed): the draw, the pair lists and from_pairs (two CSR builds and the transpose map)
    edge_set_recipe  rmat_edges + from_pairs on as many pairs
    epoch_graph      EdgeSet.from_graph(g, 1, seed = epoch) + GcnStack([128, 128, 128]).link_train_step
    epoch_recipe     rmat_edges + from_pairs + link_train_step

One JSON line per configuration:
    rmat1m    R-MAT 1 M vertices / 10 M edges

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

CONFIGS = {"rmat1m": dict(nodes=1_000_000, edges=10_000_000, feat=128, limit=420)}
NEGATIVES = (1, 5)


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

    src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(src, dst, n)            # not relabelled: the selection searches ascending rows
    del src, dst
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), deg)
    edge_keys = rows.long() * n + g.colidx.long()     # ascending: the CSR is sorted by (row, column)
    copy_r, copy_c = torch.empty_like(g.rowptr), torch.empty_like(g.colidx)
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "max_degree": int(deg.max()),
           "copy": stats(timed(lambda: (copy_r.copy_(g.rowptr), copy_c.copy_(g.colidx)))), "repeats": args.repeats, "warmup": args.warmup,
           "device": capi.device_name(0)}
    del copy_r, copy_c
    seeds = iter(range(10 ** 6))                      # a fresh seed per call
    for m in NEGATIVES:
        unfilled = []
        out[f"sampler_m{m}"] = dict(stats(timed(lambda: unfilled.append(g.sample_negatives(m, next(seeds))[1]))), unfilled=unfilled[-1])
        k = g.nnz * m
        out[f"recipe_draw_m{m}"] = stats(timed(lambda: ops.rmat_edges(next(seeds), n, k, 0.25, 0.25, 0.25, device=dev)))
        s, d = ops.rmat_edges(args.seed + 7, n, k, 0.25, 0.25, 0.25, device=dev)
        keys = s.long() * n + d.long()
        at = torch.searchsorted(edge_keys, keys).clamp(max=g.nnz - 1)
        bad = (edge_keys[at] == keys) | (s == d)
        out[f"recipe_share_m{m}"] = {"pairs": k, "edges_or_self": int(bad.sum()), "share": float(bad.double().mean())}
        del s, d, keys, at, bad
    del edge_keys

    def recipe_set(seed):
        s, d = ops.rmat_edges(seed, n, g.nnz, 0.25, 0.25, 0.25, device=dev)
        label = torch.cat([torch.zeros(g.nnz, device=dev), torch.ones(g.nnz, device=dev)])
        return ops.EdgeSet.from_pairs(torch.cat([s, rows]), torch.cat([d, g.colidx]), label, n)

    sizes = []
    out["edge_set_graph"] = stats(timed(lambda: sizes.append(ops.EdgeSet.from_graph(g, 1, next(seeds)).nnz)))
    out["edge_set_graph_pairs"] = sizes[-1]
    out["edge_set_recipe"] = stats(timed(lambda: sizes.append(recipe_set(next(seeds)).nnz)))
    out["edge_set_recipe_pairs"] = sizes[-1]
    g.make_plans(args.chunk, F)
    net = ops.GcnStack(g, [F, F, F], seed=args.seed + 100, device=dev)
    X = net.pad_input(ops.uniform_pm1(args.seed + 4, (n, F), device=dev))
    top = float(net.forward(X).abs().max())           # hub rows: keep the scores finite (the cost does not depend on values)
    if top > 4.0:
        net.W[-1].mul_(4.0 / top)
    out["link_dims"] = [F, F, F]
    out["epoch_graph"] = stats(timed(lambda: net.link_train_step(X, ops.EdgeSet.from_graph(g, 1, next(seeds)), 0.0)))
    out["epoch_recipe"] = stats(timed(lambda: net.link_train_step(X, recipe_set(next(seeds)), 0.0)))
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default="rmat1m", help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
