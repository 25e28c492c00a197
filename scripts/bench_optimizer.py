#!/usr/bin/env python3
"""Measurement (GPU box): the optimiser step of the trainable models -- `step` alone and a whole `train_step` for
GcnStack, GatStack, SageStack (mean) and GraphClassifier at the sizes of the other scripts/bench_*.py:

    gcn, gat, sage   R-MAT 1 M vertices / 10 M edges, dims [128, 128, 128] (GatStack: one head), a tenth of the rows in the loss
    clf              one batch of 5 000 graphs of 5 .. 60 vertices, SageStack([128, 128, 128], mean) + mean readout + 8 classes

for five ways to step, in the same process on the same model:

    sgd_loop       plain SGD as it was before the parameter table: one gnnx_sgd_step_f32 launch per tensor (no optimiser set)
    sgd_table      the same update through the table: ops.Momentum(momentum=0), one launch
    momentum       ops.Momentum(0.9), one launch
    adam           ops.Adam(), one launch
    adam_clipped   ops.Adam(max_grad_norm=1), the norm's two launches and the update

    step alone: --inner steps between a host clock's two readings, the second after a device synchronisation, divided by --inner;
    --repeats such windows after --warmup; the median and the range, in microseconds per step.  At these tensor sizes a step is launch
    overhead, which is what the table is about: the figure is the host's cost of a step, not a kernel time.
    train_step: single calls under the same clock, in milliseconds.

and the loss after --loss-steps training steps at the same rate (--lr) for sgd_loop and adam, each from the same initial parameters, on
the features times --loss-feature-scale: the reason to have Adam at all.

One JSON line per model.  Without --config the script is a driver: it runs every model as a child process of its own under a time limit
and stops at the first one that fails.
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

CONFIGS = {"gcn": dict(limit=300), "gat": dict(limit=300), "sage": dict(limit=300), "clf": dict(limit=300)}
NODES, EDGES, DIMS, N_GRAPHS, N_CLASSES = 1_000_000, 10_000_000, [128, 128, 128], 5000, 8


def driver(args):
    for name in args.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--inner", str(args.inner), "--loss-steps", str(args.loss_steps), "--lr", str(args.lr), "--loss-feature-scale",
               str(args.loss_feature_scale)]
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

    if args.config == "clf":
        g = torch.Generator(device="cpu").manual_seed(args.seed)
        sizes = torch.randint(5, 61, (N_GRAPHS,), generator=g)
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
        n = int(ptr[-1])
        graph = torch.repeat_interleave(torch.arange(N_GRAPHS), sizes)
        v = torch.arange(n)
        partner = ptr[graph] + torch.minimum((torch.rand(n, generator=g) * sizes[graph]).long(), sizes[graph] - 1)
        chain = v[v != ptr[graph]]
        a = torch.cat([v, partner, chain, chain - 1]).to(torch.int32).to(dev)
        b = torch.cat([partner, v, chain - 1, chain]).to(torch.int32).to(dev)
        batch = ops.GraphBatch.from_coo_batched(a, b, ptr.to(torch.int32).to(dev))
        X = ops.uniform_pm1(args.seed + 1, (batch.n, DIMS[0]), device=dev)
        target = (torch.arange(N_GRAPHS, device=dev) % N_CLASSES).to(torch.int32)
        step_args = (X, target)

        def make():
            return ops.GraphClassifier(ops.SageStack(batch, DIMS, aggr="mean", seed=args.seed + 100, device=dev), batch, N_CLASSES, pool="mean")
        shape = dict(vertices=batch.n, graphs=N_GRAPHS)
    else:
        src, dst = ops.rmat_edges(args.seed, NODES, EDGES, 0.57, 0.19, 0.19, device=dev)
        graph = ops.CsrGraph.from_coo(src, dst, NODES)
        graph.make_plans(args.chunk, max(DIMS))
        X = ops.uniform_pm1(args.seed + 1, (NODES, DIMS[0]), device=dev)
        target = (torch.arange(NODES, device=dev) % DIMS[-1]).to(torch.int32)
        mask = (torch.arange(NODES, device=dev) % 10 == 0).to(torch.uint8)
        if args.config == "gcn":
            step_args = (X, target, graph.labelled(mask))
        else:
            step_args = (X, target, graph.rows_of(mask))

        def make():
            if args.config == "gcn":
                return ops.GcnStack(graph, DIMS, seed=args.seed + 100, device=dev)
            if args.config == "gat":
                return ops.GatStack(graph, DIMS, seed=args.seed + 100, device=dev)
            return ops.SageStack(graph, DIMS, aggr="mean", seed=args.seed + 100, device=dev)
        shape = dict(nodes=NODES, edges=EDGES, nnz=graph.nnz)

    ways = {"sgd_loop": lambda: None, "sgd_table": lambda: ops.Momentum(momentum=0.0), "momentum": lambda: ops.Momentum(0.9),
            "adam": lambda: ops.Adam(), "adam_clipped": lambda: ops.Adam(max_grad_norm=1.0)}

    def clock(fn, count):
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / count

    def stats(v, scale, digits):
        return {"median": round(statistics.median(v) * scale, digits), "range": [round(min(v) * scale, digits), round(max(v) * scale, digits)]}

    net = make()
    out = {"config": args.config, **shape, "dims": DIMS, "tensors": len(net.params()), "parameters": sum(p.numel() for p in net.params()),
           "chunks_of_1024": sum(-(-p.numel() // 1024) for p in net.params()), "inner": args.inner, "repeats": args.repeats, "warmup": args.warmup,
           "device": capi.device_name(0), "step_us": {}, "train_step_ms": {}}
    del net
    for name, opt in ways.items():
        net = make().set_optimizer(opt())
        net.train_step(*step_args, 0.0)                               # real gradients, buffers allocated, the optimiser bound
        one = lambda: net.step(0.0)                                   # noqa: E731  (lr = 0: the parameters stay; same launches, same traffic)
        for _ in range(args.warmup):
            clock(one, args.inner)
        out["step_us"][name] = stats([clock(one, args.inner) for _ in range(args.repeats)], 1e6, 2)
        full = lambda: net.train_step(*step_args, 0.0)                # noqa: E731
        for _ in range(args.warmup):
            clock(full, 1)
        out["train_step_ms"][name] = stats([clock(full, 1) for _ in range(args.repeats)], 1e3, 4)
        del net
    # the loss leg runs on features scaled down: the loss has no max-subtraction (as the reference), and the hub rows of the R-MAT graph
    # push a GCN's logits on +-1 features past expf's range before any step
    out["loss"] = {"lr": args.lr, "steps": args.loss_steps, "feature_scale": args.loss_feature_scale}
    loss_args = (step_args[0] * args.loss_feature_scale,) + tuple(step_args[1:])
    for name in ("sgd_loop", "adam"):
        net = make().set_optimizer(ways[name]())
        losses = [net.train_step(*loss_args, args.lr).clone() for _ in range(args.loss_steps)]    # the loss BEFORE each step's update
        out["loss"][name] = {"first": round(float(losses[0].cpu()[0]), 5), "last": round(float(losses[-1].cpu()[0]), 5)}
        del net
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this model in this process")
    ap.add_argument("--configs", default="gcn,gat,sage,clf", help="driver mode: the models to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200, help="steps per timed window of `step` alone")
    ap.add_argument("--loss-steps", type=int, default=30)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--loss-feature-scale", type=float, default=2.0 ** -6)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
