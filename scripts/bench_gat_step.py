#!/usr/bin/env python3
"""Measurement (GPU box): the calls of a one-head GatStack layer -- the edge softmax and the transposed row sum through the multi-head
wrappers with H = 1 (ops.edge_softmax_heads / ops.edge_softmax_heads_bwd / ops.csr_rowsum_heads, as the stack makes them), the three
skinny dense products -- and one GatStack.train_step, with the PLANNED FORWARD AGGREGATION and the edge-score kernel (ops.sddmm) on the
same CSR and width in the same process as yardsticks (each of those gathers nnz * 4 F bytes of rows; the softmax moves 12 - 20 bytes
per entry).

    every kernel: --repeats single calls between two device events after --warmup calls; the median and the range are reported

One JSON line per configuration:

    rmat1m    R-MAT 1 M vertices / 10 M edges, F = 128, plus one training step of a 2-layer stack [128, 128, 128] over a tenth of the rows
    headline  R-MAT 10 M vertices / 100 M edges, F = 256 (BASELINE.md's headline graph), kernels only

The graph is NOT relabelled (CsrGraph.attention_map needs ascending rows), so the aggregation yardstick here is not BASELINE.md's
scrambled-order number.  Without --config the script is a driver: it runs every configuration as a child process of its own under a
time limit and stops at the first one that fails.  --trace N: no timing, N calls of the softmax forward and backward in a row (run
under `rocprofv3 --kernel-trace --stats -- python scripts/bench_gat_step.py --config rmat1m --trace 5` for the kernel times).

--heads (with --config rmat1m; the driver passes it on): the multi-head calls instead.  For (H, D) = (8, 8), (8, 16), (4, 32), (8, 32) one
JSON line each with ops.spmm_heads, ops.sddmm_heads, ops.edge_softmax_heads and ops.edge_softmax_heads_bwd against the loop of H
single-head calls on column slabs (the aggregation planned, as a user of the single-head call would run it; the softmax on contiguous
per-head copies, the copies in and out timed with it), then one line with a train_step of GatStack([128, 64, 16], heads=[8, 1]).
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
        if args.heads:
            cmd.append("--heads")
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
    if args.heads:
        return measure_heads(args, torch, ops, capi, g, timed)
    map_t = g.attention_map()
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    H = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    G = ops.uniform_pm1(args.seed + 2, (n, F), device=dev)
    A = ops.uniform_pm1(args.seed + 3, (2, F), scale=F ** -0.5, device=dev)
    Y = torch.empty((n, F), dtype=torch.float32, device=dev)
    dH = torch.zeros((n, F), dtype=torch.float32, device=dev)
    dA = torch.empty((2, F), dtype=torch.float32, device=dev)
    scores = torch.empty(g.nnz, dtype=torch.float32, device=dev)
    ER = ops.gemm(H, A, transB=True)
    dER = ops.uniform_pm1(args.seed + 4, (n, 2), scale=1e-3, device=dev)
    alpha = ops.edge_softmax_heads(g.rowptr, g.colidx, 1, rowterm=ER[:, :1], colterm=ER[:, 1:], negative_slope=0.2)      # [nnz, 1]
    dalpha = ops.uniform_pm1(args.seed + 5, (g.nnz, 1), device=dev)
    vals_t = torch.empty((g.nnz, 1), dtype=torch.float32, device=dev)
    d_er = torch.empty((n, 2), dtype=torch.float32, device=dev)   # the stack's dER: the softmax writes column 0, the row sum column 1
    kernels = {
        "aggregation": lambda: ops.spmm(g.rowptr, g.colidx, H, out=Y, vals=alpha.reshape(-1), plan=g.plan),
        "sddmm": lambda: ops.sddmm(g.rowptr, g.colidx, G, H, out=scores),
        "edge_softmax_fwd": lambda: ops.edge_softmax_heads(g.rowptr, g.colidx, 1, rowterm=ER[:, :1], colterm=ER[:, 1:], negative_slope=0.2),
        "edge_softmax_bwd": lambda: ops.edge_softmax_heads_bwd(g.rowptr, g.colidx, 1, alpha, dalpha, rowterm=ER[:, :1], colterm=ER[:, 1:],
                                                               negative_slope=0.2, drowterm_out=d_er[:, :1]),
        "to_transposed": lambda: ops.gather_rows(alpha, map_t, out=vals_t),
        "csr_rowsum_heads": lambda: ops.csr_rowsum_heads(g.rowptr_t, vals_t, out=d_er[:, 1:]),
        "csr_rowsum": lambda: ops.csr_rowsum(g.rowptr_t, vals_t.reshape(-1)),      # the single-head call on the same values: a yardstick
        "gemm_ER": lambda: ops.gemm(H, A, transB=True, out=ER),
        "gemm_dH_K2": lambda: ops.gemm(dER, A, out=dH, beta=1.0),
        "gemm_dA_transA": lambda: ops.gemm(dER, H, transA=True, out=dA),
    }
    if args.trace:
        for key in ("edge_softmax_fwd", "edge_softmax_bwd"):
            for _ in range(args.trace):
                kernels[key]()
        torch.cuda.synchronize()
        return 0
    ms = {k: timed(fn) for k, fn in kernels.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    model_fwd = g.nnz * 12 + n * 16          # colidx + gathered colterm + out per entry; rowptr, rowterm per row
    model_bwd = g.nnz * 20 + n * 16          # + alpha, dalpha
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "feat": F, "chunk": args.chunk,
           "max_degree": int(deg.max()), "rows_over_16": int((deg > 16).sum()), "rows_over_4096": int((deg > 4096).sum()),
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "edge_softmax_fwd_model_TBps": round(model_fwd / med["edge_softmax_fwd"] / 1e9, 3),
           "edge_softmax_bwd_model_TBps": round(model_bwd / med["edge_softmax_bwd"] / 1e9, 3),
           "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
    if cfg["step"]:
        del Y, dH, scores, G, dalpha, vals_t, d_er
        net = ops.GatStack(g, [F, F, F], seed=args.seed + 100, device=dev)
        X = ops.uniform_pm1(args.seed + 6, (n, F), device=dev)
        target = (torch.arange(n, device=dev) % F).to(torch.int32)
        rows = torch.arange(0, n, 10, device=dev, dtype=torch.int32)
        step = lambda: net.train_step(X, target, rows, 0.0)                      # noqa: E731
        t = timed(step)
        skinny = 2 * (med["gemm_ER"] + med["gemm_dH_K2"] + med["gemm_dA_transA"])
        out.update({"gat_dims": [F, F, F], "train_step_ms": [round(x, 4) for x in t], "train_step_ms_median": round(statistics.median(t), 4),
                    "skinny_products_share_of_step": round(skinny / statistics.median(t), 4)})
    print(json.dumps(out), flush=True)
    return 0


HEAD_CELLS = ((8, 8), (8, 16), (4, 32), (8, 32))


def measure_heads(args, torch, ops, capi, g, timed):
    dev, n, nnz = g.rowptr.device, g.n, g.nnz
    deg = g.rowptr[1:] - g.rowptr[:-1]
    med = lambda fn: round(statistics.median(timed(fn)), 4)   # noqa: E731
    for Hh, D in HEAD_CELLS:
        F = Hh * D
        H = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
        G = ops.uniform_pm1(args.seed + 2, (n, F), device=dev)
        ER = ops.uniform_pm1(args.seed + 3, (n, 2 * Hh), device=dev)
        dalpha = ops.uniform_pm1(args.seed + 5, (nnz, Hh), device=dev)
        alpha = ops.edge_softmax_heads(g.rowptr, g.colidx, Hh, rowterm=ER[:, :Hh], colterm=ER[:, Hh:], negative_slope=0.2)
        Y = torch.empty((n, F), dtype=torch.float32, device=dev)
        scores = torch.empty((nnz, Hh), dtype=torch.float32, device=dev)
        cols = [alpha[:, h].contiguous() for h in range(Hh)]          # the loops' per-head operands, made outside the timed calls
        outs = [torch.empty(nnz, dtype=torch.float32, device=dev) for _ in range(Hh)]
        one = torch.empty(nnz, dtype=torch.float32, device=dev)
        drow = torch.empty((n, Hh), dtype=torch.float32, device=dev)

        def agg_loop():
            for h in range(Hh):
                ops.spmm(g.rowptr, g.colidx, H[:, h * D:(h + 1) * D], out=Y[:, h * D:(h + 1) * D], vals=cols[h], plan=g.plan)

        def sddmm_loop():
            for h in range(Hh):
                ops.sddmm(g.rowptr, g.colidx, G[:, h * D:(h + 1) * D], H[:, h * D:(h + 1) * D], out=outs[h])

        def softmax_fwd_loop():   # the terms are strided views already; the entry-major result needs a copy per head
            for h in range(Hh):
                scores[:, h].copy_(ops.edge_softmax(g.rowptr, g.colidx, rowterm=ER[:, h], colterm=ER[:, Hh + h], negative_slope=0.2))

        def softmax_bwd_loop():   # contiguous copies of alpha and dalpha in, dt out
            for h in range(Hh):
                one.copy_(alpha[:, h])
                dt, dr = ops.edge_softmax_bwd(g.rowptr, g.colidx, one, dalpha[:, h].contiguous(), rowterm=ER[:, h], colterm=ER[:, Hh + h],
                                              negative_slope=0.2)
                scores[:, h].copy_(dt)
                drow[:, h].copy_(dr)

        out = {"config": args.config, "heads": Hh, "head_dim": D, "nnz": nnz, "max_degree": int(deg.max()), "ms_median": {
            "spmm_heads": med(lambda: ops.spmm_heads(g.rowptr, g.colidx, H, alpha, Hh, out=Y)),
            "spmm_loop_planned": med(agg_loop),
            "sddmm_heads": med(lambda: ops.sddmm_heads(g.rowptr, g.colidx, G, H, Hh, out=scores)),
            "sddmm_loop": med(sddmm_loop),
            "edge_softmax_heads_fwd": med(lambda: ops.edge_softmax_heads(g.rowptr, g.colidx, Hh, rowterm=ER[:, :Hh], colterm=ER[:, Hh:],
                                                                         negative_slope=0.2, out=scores)),
            "edge_softmax_fwd_loop_with_copies": med(softmax_fwd_loop),
            "edge_softmax_heads_bwd": med(lambda: ops.edge_softmax_heads_bwd(g.rowptr, g.colidx, Hh, alpha, dalpha, rowterm=ER[:, :Hh],
                                                                             colterm=ER[:, Hh:], negative_slope=0.2, drowterm_out=drow)),
            "edge_softmax_bwd_loop_with_copies": med(softmax_bwd_loop),
        }, "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
        print(json.dumps(out), flush=True)
        del H, G, ER, dalpha, alpha, Y, scores, cols, outs, one, drow
    dims, heads = [128, 64, 16], [8, 1]
    net = ops.GatStack(g, dims, seed=args.seed + 100, device=dev, heads=heads)
    X = ops.uniform_pm1(args.seed + 6, (n, dims[0]), device=dev)
    target = (torch.arange(n, device=dev) % dims[-1]).to(torch.int32)
    rows = torch.arange(0, n, 10, device=dev, dtype=torch.int32)
    t = timed(lambda: net.train_step(X, target, rows, 0.0))
    print(json.dumps({"config": args.config, "gat_dims": dims, "gat_heads": heads, "train_step_ms": [round(x, 4) for x in t],
                      "train_step_ms_median": round(statistics.median(t), 4)}), flush=True)
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
    ap.add_argument("--heads", action="store_true", help="measure the multi-head calls against the loops of single-head calls")
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
