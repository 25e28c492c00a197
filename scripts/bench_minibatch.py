#!/usr/bin/env python3
"""Measurement (GPU box): mini-batch GraphSAGE on a sampled field (CsrGraph.sampled_field + SageStack.batch_step, DESIGN.md section
5.10), SageStack([128, 128, 128]), batch 1024, fanouts [10, 10] and [25, 10], aggr = mean.

    every figure: single calls under a host clock that ends in a device synchronisation, after --warmup calls of the same shape; the
    median and the range of --repeats calls are reported.  Each call uses a batch and a seed of its own (a fixed schedule).
    one process per graph; within it the two sides of a comparison alternate round by round: baseline, mini-batch, baseline again.

Per fanout list:
    field          g.sampled_field(batch, fanouts, seed), and its parts summed over the layers, timed one by one in a second pass over
                   the same calls: sampler (sample_rows), frontier (mask to rows + position table: the O(n) part), renumber,
                   transposed (csr_from_coo of the block's COO); `rest` is what the class does besides (seeds' rows, self_pos, inv_deg)
    batch_step     net.batch_step on a field that is already built
    minibatch      field + batch_step, as a user runs it
    baseline_a/b   what the parent commit offers for the same batch: net.on_graph(g.sample_neighbors(k, seed)).train_step(X, target,
                   batch_rows, lr) with k = max(fanouts), its sample_neighbors included -- before and after the mini-batch leg
    rows, nnz      |Q_l| and the kept entries per layer, means over the timed batches
and once per graph:
    o_n            the O(n) work of one layer with nothing listed: a zeroed [n] mark, gnnx_mask_to_rows over it, the position table's fill
    sample_rows_*  ops.sample_rows against ops.sample_neighbors (k = 10, rowid on) for lists of 1 000, 100 000 and n rows

One JSON line per configuration:
    rmat1m    R-MAT 1 M vertices / 10 M edges
    headline  R-MAT 10 M vertices / 100 M edges (BASELINE.md's headline graph)

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

CONFIGS = {"rmat1m": dict(nodes=1_000_000, edges=10_000_000, limit=300),
           "headline": dict(nodes=10_000_000, edges=100_000_000, limit=540)}
FANOUTS = ([10, 10], [25, 10])
BATCH, F = 1024, 128
PARTS = ("sampler", "frontier", "renumber", "transposed")


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

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ms):
        return {"ms_median": round(statistics.median(ms), 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)]}

    src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(src, dst, n)
    del src, dst
    g.make_plans(args.chunk, F)
    X = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    target = (torch.arange(n, device=dev) % F).to(torch.int32)
    net = ops.SageStack(g, [F, F, F], aggr="mean", seed=args.seed + 100, device=dev)
    gen = torch.Generator().manual_seed(args.seed)
    rounds = args.warmup + args.repeats
    batches = [torch.randint(0, n, (BATCH,), generator=gen).to(dev) for _ in range(rounds)]
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "batch": BATCH, "sage_dims": [F, F, F], "repeats": args.repeats,
           "warmup": args.warmup, "device": capi.device_name(0)}

    def field_parts(batch, fanouts, seed):
        """SampledField's calls, layer by layer, each under the clock"""
        ms = dict.fromkeys(PARTS, 0.0)
        L = len(fanouts)
        mark = torch.zeros(n, dtype=torch.uint8, device=dev)
        mark[batch] = 1
        rows = ops.rows_from_mask(mark)
        for l in range(L, 0, -1):
            t, (rp, ci, _, rowid) = clocked(lambda: ops.sample_rows(g.rowptr, g.colidx, rows, fanouts[l - 1], seed * L + l - 1, n_cols=n,
                                                                     want_rowid=True, col_mark=mark))
            ms["sampler"] += t
            t, (below, pos) = clocked(lambda: (lambda b: (b, ops.rows_to_positions(b, n)))(ops.rows_from_mask(mark)))
            ms["frontier"] += t
            ms["renumber"] += clocked(lambda: ops.renumber_cols(ci, pos))[0]
            ms["transposed"] += clocked(lambda: ops.CsrGraph.csr_from_coo(ci, rowid, int(below.numel()), flags=3))[0]
            rows = below
        return ms

    for fanouts in FANOUTS:
        k = max(fanouts)
        tag = "x".join(str(v) for v in fanouts)
        legs = {name: [] for name in ("field", "batch_step", "minibatch", "baseline_a", "baseline_b") + PARTS}
        sizes = []

        def baseline(it):
            rows = ops.rows_from_mask(torch.zeros(n, dtype=torch.uint8, device=dev).index_fill_(0, batches[it], 1))
            return clocked(lambda: net.on_graph(g.sample_neighbors(k, it)).train_step(X, target, rows, 0.0))[0]

        for it in range(rounds):
            a = baseline(it)
            t_field, field = clocked(lambda: g.sampled_field(batches[it], fanouts, seed=it))
            t_step = clocked(lambda: net.batch_step(X, target, field, 0.0))[0]
            b = baseline(it)
            parts = field_parts(batches[it], fanouts, it)
            if it >= args.warmup:
                for name, v in (("field", t_field), ("batch_step", t_step), ("minibatch", t_field + t_step), ("baseline_a", a), ("baseline_b", b)):
                    legs[name].append(v)
                for name in PARTS:
                    legs[name].append(parts[name])
                sizes.append(([int(r.numel()) for r in field.rows], field.nnz))
            del field
        res = {name: stats(v) for name, v in legs.items()}
        res["rest"] = round(res["field"]["ms_median"] - sum(res[p]["ms_median"] for p in PARTS), 4)
        res["baseline_k"] = k
        res["rows_mean"] = [round(statistics.mean(s[0][l] for s in sizes), 1) for l in range(len(fanouts) + 1)]
        res["nnz_mean"] = [round(statistics.mean(s[1][l] for s in sizes), 1) for l in range(len(fanouts) + 1)]
        out[f"fanouts_{tag}"] = res

    def o_n():
        mark = torch.zeros(n, dtype=torch.uint8, device=dev)
        ops.rows_to_positions(ops.rows_from_mask(mark), n)
    for _ in range(args.warmup):
        o_n()
    out["o_n"] = stats([clocked(o_n)[0] for _ in range(args.repeats)])

    def listed(m):
        rows = torch.randint(0, n, (m,), generator=gen).to(dev).to(torch.int32) if m < n else torch.arange(n, dtype=torch.int32, device=dev)
        fn = lambda: ops.sample_rows(g.rowptr, g.colidx, rows, 10, 3, n_cols=n, want_rowid=True)  # noqa: E731
        for _ in range(args.warmup):
            fn()
        return stats([clocked(fn)[0] for _ in range(args.repeats)])
    for m in (1_000, 100_000, n):
        out[f"sample_rows_{m if m < n else 'n'}"] = listed(m)
    whole = lambda: ops.sample_neighbors(g.rowptr, g.colidx, 10, 3, want_rowid=True)  # noqa: E731
    for _ in range(args.warmup):
        whole()
    out["sample_neighbors"] = stats([clocked(whole)[0] for _ in range(args.repeats)])
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default="rmat1m,headline", help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
