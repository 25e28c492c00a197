#!/usr/bin/env python3
"""Measurement (GPU box): the graph readout, ops.segment_pool / ops.segment_pool_bwd (gnnx_segment_pool_f32), at
1 M rows x 128 features for three segment shapes:

    short   50 000 segments of mean length 20 (49 999 random cut points: lengths from 1 to a few hundred)
    eight   8 segments of 125 000 rows
    one     one segment of 1 M rows

    every figure: --repeats single calls after --warmup calls under a host clock, each followed by a device synchronisation inside the
    clock; the median and the range are reported, in ms

Beside the readout, in the same process and on the same data:
    identity CSR   what the library offered before: the readout as an aggregation on the CSR whose row b lists the columns
                   segptr[b] .. segptr[b+1] - 1 -- ops.spmm for sum (rowscale = 1 / len for mean), ops.spmm_reduce for max; backward on the
                   transposed CSR (one entry per row: the vertex's graph) -- ops.spmm (colscale = 1 / len for mean), ops.spmm_reduce_bwd
                   with the transpose map.  Its construction (column list, transposed CSR, transpose map, plans for the long rows) is
                   reported separately as `identity_build`: it is per batch.
    copy           a device copy of X: the traffic yardstick.  A copy moves 2x the bytes the forward reads.
and with --config epoch one GraphClassifier epoch over 10 batches of 5 000 small graphs (5 .. 60 vertices) through clf.on_batch:
SageStack([128, 128, 128], mean) + mean readout + 8 classes; the construction of the 10 GraphBatch objects is reported beside it.

One JSON line per configuration.  Without --config the script is a driver: it runs every configuration as a child process of its own
under a time limit and stops at the first one that fails.
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

CONFIGS = {"kernels": dict(limit=420), "epoch": dict(limit=300)}
N_ROWS, F = 1_000_000, 128
OPS = ("sum", "mean", "max")


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
    gen = torch.Generator(device="cpu").manual_seed(args.seed)

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

    out = {"config": args.config, "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
    if args.config == "kernels":
        out.update(rows=N_ROWS, features=F)
        X = ops.uniform_pm1(args.seed + 1, (N_ROWS, F), device=dev)
        Xc = torch.empty_like(X)
        out["copy"] = stats(timed(lambda: Xc.copy_(X)))
        del Xc
        cuts = torch.sort(torch.randperm(N_ROWS - 1, generator=gen)[:49_999] + 1).values          # 50 000 segments, none empty
        short = torch.diff(torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([N_ROWS])]))
        assert int(short.min()) >= 1 and int(short.numel()) == 50_000
        shapes = {"short": short, "eight": torch.full((8,), N_ROWS // 8), "one": torch.tensor([N_ROWS])}
        for name, lens in shapes.items():
            segptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32).to(dev)
            n_seg = int(lens.numel())
            assert int(segptr[-1]) == N_ROWS
            G = ops.uniform_pm1(args.seed + 2, (n_seg, F), device=dev)
            Y = torch.empty((n_seg, F), dtype=torch.float32, device=dev)
            arg = torch.empty((n_seg, F), dtype=torch.int32, device=dev)
            dX = torch.empty_like(X)
            res = {"segments": n_seg, "longest": int(lens.max())}
            for op in OPS:
                res[f"pool_{op}"] = stats(timed(lambda: ops.segment_pool(segptr, X, op, out=Y, arg_out=arg)))
                res[f"pool_bwd_{op}"] = stats(timed(lambda: ops.segment_pool_bwd(segptr, G, op, arg=arg, out=dX)))
            built = {}

            def build():
                colidx = torch.arange(N_ROWS, dtype=torch.int32, device=dev)
                rowptr_t = torch.arange(N_ROWS + 1, dtype=torch.int32, device=dev)
                colidx_t = torch.repeat_interleave(torch.arange(n_seg, dtype=torch.int32, device=dev), (segptr[1:] - segptr[:-1]).long())
                map_t = ops.csr_transpose_map(segptr, colidx, rowptr_t, colidx_t)
                inv_len = (1.0 / (segptr[1:] - segptr[:-1]).to(torch.float32))
                built.update(colidx=colidx, rowptr_t=rowptr_t, colidx_t=colidx_t, map_t=map_t, inv_len=inv_len,
                             plan=ops.SpmmPlan(segptr, args.chunk, F), plan_t=ops.SpmmPlan(rowptr_t, args.chunk, F))
            res["identity_build"] = stats(timed(build))
            b = built
            res["identity_sum"] = stats(timed(lambda: ops.spmm(segptr, b["colidx"], X, out=Y, plan=b["plan"])))
            res["identity_mean"] = stats(timed(lambda: ops.spmm(segptr, b["colidx"], X, out=Y, rowscale=b["inv_len"], plan=b["plan"])))
            res["identity_max"] = stats(timed(lambda: ops.spmm_reduce(segptr, b["colidx"], X, op="max", out=Y, arg_out=arg)))
            res["identity_bwd_sum"] = stats(timed(lambda: ops.spmm(b["rowptr_t"], b["colidx_t"], G, out=dX, plan=b["plan_t"])))
            res["identity_bwd_mean"] = stats(timed(lambda: ops.spmm(b["rowptr_t"], b["colidx_t"], G, out=dX, colscale=b["inv_len"],
                                                                    plan=b["plan_t"])))
            res["identity_bwd_max"] = stats(timed(lambda: ops.spmm_reduce_bwd(b["rowptr_t"], b["colidx_t"], b["map_t"], arg, G, out=dX)))
            out[name] = res
            del built, b, dX
    else:
        n_batches, n_graphs, d, n_classes = 10, 5000, 128, 8
        out.update(batches=n_batches, graphs_per_batch=n_graphs, sage_dims=[d, d, d], pool="mean", classes=n_classes)

        def edges(k):
            """graphs of 5 .. 60 vertices: every vertex but a graph's first is tied to its predecessor and every vertex to one random
            vertex of its own graph, both directions"""
            g = torch.Generator(device="cpu").manual_seed(args.seed + k)
            sizes = torch.randint(5, 61, (n_graphs,), generator=g)
            ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
            n = int(ptr[-1])
            graph = torch.repeat_interleave(torch.arange(n_graphs), sizes)
            v = torch.arange(n)
            partner = ptr[graph] + torch.minimum((torch.rand(n, generator=g) * sizes[graph]).long(), sizes[graph] - 1)
            chain = v[v != ptr[graph]]
            a = torch.cat([v, partner, chain, chain - 1]).to(torch.int32).to(dev)
            b = torch.cat([partner, v, chain - 1, chain]).to(torch.int32).to(dev)
            return a, b, ptr.to(torch.int32).to(dev), n

        lists = [edges(k) for k in range(n_batches)]
        batches = []

        def build_batches():
            batches.clear()
            for a, b, ptr, _ in lists:
                batches.append(ops.GraphBatch.from_coo_batched(a, b, ptr))
        out["batch_build_all"] = stats(timed(build_batches))
        out["vertices"] = [b.n for b in batches]
        Xs = [ops.uniform_pm1(args.seed + 50 + k, (b.n, d), device=dev) for k, b in enumerate(batches)]
        targets = [(torch.arange(b.n_graphs, device=dev) % n_classes).to(torch.int32) for b in batches]
        clf = ops.GraphClassifier(ops.SageStack(batches[0], [d, d, d], aggr="mean", seed=args.seed + 100, device=dev), batches[0], n_classes,
                                  pool="mean")

        def epoch():
            for b, X, t in zip(batches, Xs, targets):
                clf.on_batch(b).train_step(X, t, 0.0)
        out["epoch"] = stats(timed(epoch))
        views = [clf.on_batch(b) for b in batches]

        def epoch_bound():
            for c, X, t in zip(views, Xs, targets):
                c.train_step(X, t, 0.0)
        out["epoch_views_kept"] = stats(timed(epoch_bound))
        c0 = views[0]
        H = c0.net.forward(Xs[0])
        Z = torch.empty((batches[0].n_graphs, d), dtype=torch.float32, device=dev)
        out["readout_fwd_one_batch"] = stats(timed(lambda: ops.segment_pool(batches[0].graph_ptr, H, "mean", out=Z)))
        out["readout_bwd_one_batch"] = stats(timed(lambda: ops.segment_pool_bwd(batches[0].graph_ptr, Z, "mean", out=c0.net.grad_buffer())))
        out["step_one_batch"] = stats(timed(lambda: c0.train_step(Xs[0], targets[0], 0.0)))
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default="kernels,epoch", help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
