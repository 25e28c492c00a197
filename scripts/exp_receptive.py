#!/usr/bin/env python3
"""Measurement (GPU box): logits of a query set from its L-hop receptive field (GcnStack.predict on CsrGraph.receptive_field)
against the full forward, in ONE process with the variants alternated:

    forward (A) | predict | forward (B), each a block of --steps calls between two device events, --rounds times

The spread of the run is |forward A - forward B| (the same code measured twice).  Per query: |Q_l| and the block entries per layer,
the one-off receptive_field build (wall, after a warm-up build), predict and forward in ms, and whether predict has the bits of the
forward on the query's rows.  One JSON line per (dims, query).  --trace N: no timing, N field builds and N predicts per query (run
under `rocprofv3 --kernel-trace --stats -- python scripts/exp_receptive.py --trace 5 ...` for the marking / extraction kernel times).

Defaults: R-MAT 1 M vertices / 10 M edges, scrambled order, plans with chunk 1024 (as scripts/bench_masked_step.py), 2 layers,
dims [128, 128, 128] and [128, 128, 47]; --graph uniform draws the same number of uniform edges instead.
Queries: one ordinary vertex, 1 000 random vertices, 1 % of the vertices, the top hub.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

load_package()
ops = importlib.import_module("gnncpp_amd.ops")
capi = importlib.import_module("gnncpp_amd.capi")
dev = torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed_block(fn, reps):
    """ms per call of fn over `reps` calls between two device events"""
    a, b = capi.Event(), capi.Event()
    a.record(stream())
    for _ in range(reps):
        fn()
    b.record(stream())
    b.sync()
    return a.elapsed_ms(b) / reps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="rmat", choices=["rmat", "uniform"])
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--classes", default="128,47", help="outputs of the last layer, one stack per value")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--relabel", default="scramble", choices=["scramble", "none"])
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n, e, F, L = args.nodes, args.edges, args.feat, args.layers

    if args.graph == "rmat":
        src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    else:
        gen = torch.Generator(device="cpu").manual_seed(args.seed)
        src = torch.randint(0, n, (e,), generator=gen, dtype=torch.int32).to(dev)
        dst = torch.randint(0, n, (e,), generator=gen, dtype=torch.int32).to(dev)
    relabel = None if args.relabel == "none" else args.relabel
    g = ops.CsrGraph.from_coo(src, dst, n, relabel=relabel)
    del src, dst
    if args.chunk > 0:
        g.make_plans(args.chunk, F)
    deg = g.to_vertex_order(g.rowptr[1:] - g.rowptr[:-1])
    gen = torch.Generator(device="cpu").manual_seed(args.seed + 7)
    perm = torch.randperm(n, generator=gen)
    ordinary = int(perm[((deg.cpu()[perm] > 0) & (deg.cpu()[perm] < 64)).nonzero()[0]])
    queries = [("1 vertex", torch.tensor([ordinary])), ("1000 random", perm[:1000].clone()), ("1 %", perm[: n // 100].clone()),
               ("top hub", torch.argmax(deg).reshape(1).cpu())]

    for Cn in [int(c) for c in args.classes.split(",")]:
        dims = [F] * L + [Cn]
        net = ops.GcnStack(g, dims, seed=args.seed + 100, device=dev)
        X = net.pad_input(ops.uniform_pm1(args.seed + 1, (n, F), device=dev))
        for name, q in queries:
            q = q.to(dev).long()
            g.receptive_field(q, L)                                         # warm-up of the build kernels and the scratch buffers
            field, ms_build = wall(lambda: g.receptive_field(q, L))
            if args.trace:
                for _ in range(args.trace):
                    g.receptive_field(q, L)
                for _ in range(args.trace):
                    net.predict(X, field)
                torch.cuda.synchronize()
                continue
            same_bits = bool(torch.equal(net.predict(X, field), net.forward(X)[field.query_rows.long()]))
            variants = {"forward_a": lambda: net.forward(X), "predict": lambda: net.predict(X, field), "forward_b": lambda: net.forward(X)}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            ms = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed_block(fn, args.steps))
            med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
            print(json.dumps({
                "graph": args.graph, "nodes": n, "edges": e, "nnz": g.nnz, "dims": dims, "relabel": args.relabel, "chunk": args.chunk,
                "query": name, "n_query": field.n_query, "field_rows": [int(r.numel()) for r in field.rows], "field_nnz": list(field.nnz),
                "field_build_ms": round(ms_build, 3), "ms_median": med, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                "spread_ms": round(abs(med["forward_a"] - med["forward_b"]), 4), "same_bits": same_bits,
                "steps": args.steps, "rounds": args.rounds, "device": capi.device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
