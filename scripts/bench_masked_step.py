#!/usr/bin/env python3
"""Measurement (GPU box): the semi-supervised training step of ops.GcnStack with the last layer pruned to the labelled rows
(train_step with a LabelledSet) against the same masked step on the full CSR, in ONE process with the variants alternated:

    unpruned (A) | pruned | unpruned (B) | unmasked, each a block of --steps steps between two device events, --rounds times

The spread of the run is |unpruned A - unpruned B| (the same code measured twice).  Also: the two last-layer aggregations alone
(full CSR vs restricted CSR), the one-off cost of CsrGraph.labelled(mask) next to CsrGraph.from_coo, and the kept-entry share.
One JSON line per label fraction.  --trace N: no timing, N steps of each variant in a row (run under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_masked_step.py --trace 5 ...` for the kernel times).

Defaults: BASELINE config [2] (R-MAT 1 M vertices / 10 M edges), a 2-layer stack [128, 128, 128] as bench.py --train-layers 2
builds it (scrambled labels, plans with chunk 1024); --classes 47 gives the last layer 47 outputs.
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
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--classes", type=int, default=0, help="outputs of the last layer (0: --feat)")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--fractions", default="0.01,0.1")
    ap.add_argument("--hubs-labelled", type=int, default=0, help="also label the K vertices of highest degree")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--relabel", default="scramble", choices=["scramble", "none"])
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n, e, F = args.nodes, args.edges, args.feat
    Cn = args.classes or F
    dims = [F] * args.layers + [Cn]

    src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    relabel = None if args.relabel == "none" else args.relabel
    ops.CsrGraph.from_coo(src, dst, n, relabel=relabel)                     # warm-up of the build kernels
    g, ms_from_coo = wall(lambda: ops.CsrGraph.from_coo(src, dst, n, relabel=relabel))
    del src, dst
    if args.chunk > 0:
        g.make_plans(args.chunk, max(dims))
    net = ops.GcnStack(g, dims, seed=args.seed + 100, device=dev)
    X = net.pad_input(ops.uniform_pm1(args.seed + 1, (n, F), device=dev))
    # logits of a hub row stay finite without max-subtraction: small last weights (the step's cost does not depend on the values)
    top = float(net.forward(X).abs().max())
    if top > 8.0:
        net.W[-1].mul_(8.0 / top)
    target_all = (torch.arange(n, device=dev, dtype=torch.int64) * 7 + 3).remainder(Cn).to(torch.int32)
    deg = g.to_vertex_order(g.rowptr[1:] - g.rowptr[:-1])

    for frac in [float(f) for f in args.fractions.split(",")]:
        gen = torch.Generator(device="cpu").manual_seed(args.seed + 7)
        mask = torch.zeros(n, dtype=torch.uint8)
        mask[torch.randperm(n, generator=gen)[: int(round(frac * n))]] = 1
        mask = mask.to(dev)
        if args.hubs_labelled:
            mask[torch.topk(deg, args.hubs_labelled).indices] = 1
        g.labelled(mask)                                                    # warm-up
        lab, ms_labelled = wall(lambda: g.labelled(mask))
        target = torch.where(g.to_new_order(mask) != 0, target_all, torch.full_like(target_all, -1))
        lr = 1e-3

        def unmasked():
            logits = net.forward(X)
            # (grad_buffer() drops the stack's zeroed-rows mark: the buffer now holds every row)
            _, dlog = ops.softmax_ce(logits, target_all, colsum_out=net.db[-1], grad_out=net.grad_buffer())
            net.backward(dlog, input_grad=False, have_last_bias_grad=True)
            net.step(lr)

        def unpruned():   # train_step's calls with both last-layer aggregations on the full CSR (same bits)
            logits = net.forward(X)
            _, dlog = ops.softmax_ce_rows(logits, target, lab.rows, colsum_out=net.db[-1], grad_out=net.masked_grad_buffer(lab))
            net.backward(dlog, input_grad=False, have_last_bias_grad=True)
            net.step(lr)

        variants = {"unpruned_a": unpruned, "pruned": lambda: net.train_step(X, target, lab, lr), "unpruned_b": unpruned,
                    "unmasked": unmasked}
        if args.trace:
            for fn in variants.values():
                for _ in range(args.trace):
                    fn()
            torch.cuda.synchronize()
            continue
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(timed_block(fn, args.steps))
        # the two last-layer aggregations alone
        H = ops.uniform_pm1(5, (n, Cn), device=dev)
        G = net.masked_grad_buffer(lab)
        agg = {}
        for name, fn in (("fwd_full", lambda: ops.aggregate_fwd(g, H, net.b[-1])),
                         ("fwd_restricted", lambda: ops.aggregate_fwd(g, H, net.b[-1], labelled=lab)),
                         ("bwd_full", lambda: ops.aggregate_bwd(g, G)),
                         ("bwd_restricted", lambda: ops.aggregate_bwd(g, G, labelled=lab))):
            for _ in range(args.warmup):
                fn()
            agg[name] = round(timed_block(fn, args.steps), 4)
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        print(json.dumps({
            "nodes": n, "edges": e, "nnz": g.nnz, "dims": dims, "relabel": args.relabel, "chunk": args.chunk,
            "label_fraction": frac, "hubs_labelled": args.hubs_labelled, "n_labelled": lab.n_labelled,
            "kept_entries": lab.nnz, "kept_share": round(lab.nnz / max(g.nnz, 1), 4),
            "step_ms_median": med, "step_ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "spread_ms": round(abs(med["unpruned_a"] - med["unpruned_b"]), 4),
            "gain_ms": round((med["unpruned_a"] + med["unpruned_b"]) / 2 - med["pruned"], 4),
            "last_layer_aggregation_ms": agg,
            "from_coo_ms": round(ms_from_coo, 2), "labelled_ms": round(ms_labelled, 2),
            "steps": args.steps, "rounds": args.rounds, "device": capi.device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
