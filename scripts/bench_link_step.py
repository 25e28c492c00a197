#!/usr/bin/env python3
"""Measurement (GPU box): the edge-score kernel (ops.sddmm, gnnx_sddmm_csr_f32) against the PLANNED FORWARD AGGREGATION on the same CSR
and width in the same process -- that kernel gathers the same nnz * 4 F bytes of rows -- and one link-prediction step
(GcnStack.link_train_step).

    aggregation (A) | sddmm | aggregation (B), each --repeats single calls between two device events after --warmup calls

The aggregation's own run-to-run spread is the range of its 2 * --repeats times; ratio = median(sddmm) / median(aggregation).  One JSON
line per configuration:

    rmat1m    R-MAT 1 M vertices / 10 M edges, F = 128, plus the link step (a 2-layer stack [128, 128, 128]; positives = every
              second edge, as many uniform negatives listed before them)
    headline  R-MAT 10 M vertices / 100 M edges, F = 256 (BASELINE.md's headline graph)

Without --config the script is a driver: it runs every configuration as a child process of its own under a time limit and stops at
the first one that fails.  --trace N: no timing, N calls of each kernel in a row (run under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_link_step.py --config rmat1m --trace 5` for the kernel times).
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

CONFIGS = {"rmat1m": dict(nodes=1_000_000, edges=10_000_000, feat=128, link=True, limit=300),
           "headline": dict(nodes=10_000_000, edges=100_000_000, feat=256, link=False, limit=420)}


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

    src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(src, dst, n, relabel="scramble")
    g.make_plans(args.chunk, F)
    H = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    Lm = ops.uniform_pm1(args.seed + 2, (n, F), device=dev)
    Y = torch.empty((n, F), dtype=torch.float32, device=dev)
    scores = torch.empty(g.nnz, dtype=torch.float32, device=dev)
    agg = lambda: ops.aggregate_fwd(g, H, out=Y)                                 # noqa: E731
    sddmm = lambda: ops.sddmm(g.rowptr, g.colidx, Lm, H, out=scores)             # noqa: E731
    if args.trace:
        for fn in (agg, sddmm):
            for _ in range(args.trace):
                fn()
        torch.cuda.synchronize()
        return 0
    ms = {"agg_a": [], "sddmm": [], "agg_b": []}
    for key, fn in (("agg_a", agg), ("sddmm", sddmm), ("agg_b", agg)):
        for _ in range(args.warmup):
            fn()
        ms[key] = [one_call_ms(fn) for _ in range(args.repeats)]
    agg_all = ms["agg_a"] + ms["agg_b"]
    agg_med, sd_med = statistics.median(agg_all), statistics.median(ms["sddmm"])
    gathered = g.nnz * 4 * F
    model = g.nnz * (4 * F + 8) + 4 * F * n + 4 * g.nnz
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "feat": F, "chunk": args.chunk,
           "aggregation_ms": [round(x, 4) for x in agg_all], "sddmm_ms": [round(x, 4) for x in ms["sddmm"]],
           "aggregation_ms_median": round(agg_med, 4), "sddmm_ms_median": round(sd_med, 4),
           "aggregation_spread_ms": round(max(agg_all) - min(agg_all), 4), "ratio_sddmm_to_aggregation": round(sd_med / agg_med, 4),
           "aggregation_spread_rel": round((max(agg_all) - min(agg_all)) / agg_med, 4),
           "sddmm_gathered_TBps": round(gathered / sd_med / 1e9, 3), "sddmm_model_TBps": round(model / sd_med / 1e9, 3),
           "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
    if cfg["link"]:
        del Y, scores, Lm
        pos_s, pos_d = src[::2].contiguous(), dst[::2].contiguous()
        k = int(pos_s.numel())
        neg_s, neg_d = ops.rmat_edges(args.seed + 3, n, k, 0.25, 0.25, 0.25, device=dev)
        nid = g.nid.long()                                                      # pairs in the graph's row order
        ps, pd = nid[torch.cat([neg_s, pos_s]).long()].to(torch.int32), nid[torch.cat([neg_d, pos_d]).long()].to(torch.int32)
        label = torch.cat([torch.zeros(k, device=dev), torch.ones(k, device=dev)])
        edges = ops.EdgeSet.from_pairs(ps, pd, label, n)
        net = ops.GcnStack(g, [F, F, F], seed=args.seed + 100, device=dev)
        X = net.pad_input(ops.uniform_pm1(args.seed + 4, (n, F), device=dev))
        top = float(net.forward(X).abs().max())                                 # hub rows: keep the scores finite (the cost does not depend on values)
        if top > 4.0:
            net.W[-1].mul_(4.0 / top)
        step = lambda: net.link_train_step(X, edges, 0.0)                       # noqa: E731
        for _ in range(args.warmup):
            step()
        t = [one_call_ms(step) for _ in range(args.repeats)]
        out.update({"link_pairs": edges.nnz, "link_dims": [F, F, F], "link_train_step_ms": [round(x, 4) for x in t],
                    "link_train_step_ms_median": round(statistics.median(t), 4)})
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default="rmat1m,headline", help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
