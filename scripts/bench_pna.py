#!/usr/bin/env python3
"""Measurement (GPU box): the PNA aggregation -- ops.spmm_pna (mean | min | max | std from one gather) and ops.spmm_pna_bwd (coefficient
kernel + one walk of the transposed rows) -- against the compositions of existing calls they replace, in one process:

    forward composition    spmm(X, rowscale = 1 / deg)  +  binary("mul", X, X)  +  spmm(X * X, rowscale)  +  spmm_reduce max  +  spmm_reduce min
                           (the element-wise sqrt(msq - mean^2 + eps) that would still follow is NOT timed: the composition is favoured)
    backward composition   spmm(dmean, colscale) + spmm(dstd, colscale, beta = 1) on CSR(A^T)  +  2 x spmm_reduce_bwd(beta = 1)
                           (the x_c (.) sum B product that would still follow is NOT timed)
    train_step             PnaStack([F, F, F]) next to SageStack([F, F, F], aggr = "mean") on every third row

    every kernel: --repeats single calls between two device events after --warmup calls; the median and the range are reported

Byte model, per call, against the 8 TB/s HBM specification (every matrix counted once, although gathered rows come from cache):
    spmm_pna        nnz * (4 F [X row] + 4 [colidx])  +  n * (16 F [M] + 8 F [args] + 4 [rowptr])
    composition     nnz * (16 F + 16)  +  n * (8 F [X read, X * X written] + 16 F [four outputs] + 8 F [args] + 16)
    spmm_pna_bwd    n * (16 F [M, dM: mean and std slabs] + 8 F [A, B] + 4)  +  nnz * (24 F [A, B, two args, dmax, dmin rows] + 8)  +  n * (12 F + 4)
    composition     nnz * (16 F [dmean, dstd, dmax, dmin rows] + 8 F [two args] + 24)  +  n * (4 F [first store] + 3 * 8 F [beta = 1] + 16)

One JSON line per configuration: rmat1m_f64 / rmat1m_f128 -- R-MAT 1 M vertices / 10 M edges, symmetrised.  Without --config the script
is a driver: it runs every configuration as a child process of its own under a time limit and stops at the first one that fails.
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

CONFIGS = {"rmat1m_f64": dict(nodes=1_000_000, edges=10_000_000, feat=64, limit=300),
           "rmat1m_f128": dict(nodes=1_000_000, edges=10_000_000, feat=128, limit=300)}
HBM_SPEC_TBPS = 8.0


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
    n, F = cfg["nodes"], cfg["feat"]

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

    src, dst = ops.rmat_edges(args.seed, n, cfg["edges"], 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(torch.cat([src, dst]), torch.cat([dst, src]), n)          # symmetrised
    nnz, map_t = g.nnz, g.attention_map()
    deg = g.rowptr[1:] - g.rowptr[:-1]
    inv_deg = torch.where(deg > 0, 1.0 / deg.clamp(min=1).float(), torch.zeros((), device=dev)).contiguous()
    X = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    dM = ops.uniform_pm1(args.seed + 2, (n, 4 * F), device=dev)
    M, amin, amax = ops.spmm_pna(g.rowptr, g.colidx, X)
    X2, dX = torch.empty_like(X), torch.empty_like(X)
    mean, msq, mx, mn = (torch.empty_like(X) for _ in range(4))
    a1, a2 = (torch.empty((n, F), dtype=torch.int32, device=dev) for _ in range(2))
    dmean, dmin, dmax, dstd = (dM[:, k * F:(k + 1) * F] for k in range(4))

    def fwd_composed():
        ops.spmm(g.rowptr, g.colidx, X, out=mean, rowscale=inv_deg)
        ops.binary("mul", X, X, out=X2)
        ops.spmm(g.rowptr, g.colidx, X2, out=msq, rowscale=inv_deg)
        ops.spmm_reduce(g.rowptr, g.colidx, X, op="max", out=mx, arg_out=a1)
        ops.spmm_reduce(g.rowptr, g.colidx, X, op="min", out=mn, arg_out=a2)

    def bwd_composed():
        ops.spmm(g.rowptr_t, g.colidx_t, dmean, out=dX, colscale=inv_deg)
        ops.spmm(g.rowptr_t, g.colidx_t, dstd, out=dX, colscale=inv_deg, beta=1.0)
        ops.spmm_reduce_bwd(g.rowptr_t, g.colidx_t, map_t, amax, dmax, out=dX, beta=1.0)
        ops.spmm_reduce_bwd(g.rowptr_t, g.colidx_t, map_t, amin, dmin, out=dX, beta=1.0)

    kernels = {
        "spmm_pna": lambda: ops.spmm_pna(g.rowptr, g.colidx, X, out=M, argmin_out=amin, argmax_out=amax),
        "fwd_composed": fwd_composed,
        "spmm_pna_bwd": lambda: ops.spmm_pna_bwd(g.rowptr_t, g.colidx_t, map_t, g.rowptr, X, M, amin, amax, dM, out=dX),
        "bwd_composed": bwd_composed,
        "spmm_floor": lambda: ops.spmm(g.rowptr, g.colidx, X, out=mean),
    }
    ms = {k: timed(fn) for k, fn in kernels.items()}
    rows = torch.arange(0, n, 3, device=dev, dtype=torch.int32)
    target = (torch.arange(n, device=dev) % F).to(torch.int32)
    for name, net in (("pna_train_step", ops.PnaStack(g, [F, F, F], seed=args.seed + 100, device=dev)),
                      ("sage_mean_train_step", ops.SageStack(g, [F, F, F], aggr="mean", seed=args.seed + 100, device=dev))):
        ms[name] = timed(lambda: net.train_step(X, target, rows, 0.0))
    med = {k: statistics.median(v) for k, v in ms.items()}
    model = {"spmm_pna": nnz * (4 * F + 4) + n * (24 * F + 4),
             "fwd_composed": nnz * (16 * F + 16) + n * (32 * F + 16),
             "spmm_pna_bwd": n * (24 * F + 4) + nnz * (24 * F + 8) + n * (12 * F + 4),
             "bwd_composed": nnz * (24 * F + 24) + n * (28 * F + 16),
             "spmm_floor": nnz * (4 * F + 4) + n * (4 * F + 4)}
    out = {"config": args.config, "nodes": n, "nnz": nnz, "feat": F, "max_degree": int(deg.max()), "rows_over_4096": int((deg > 4096).sum()),
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "fwd_composed_over_fused": round(med["fwd_composed"] / med["spmm_pna"], 3),
           "bwd_composed_over_fused": round(med["bwd_composed"] / med["spmm_pna_bwd"], 3),
           "model_TBps": {k: round(b / med[k] / 1e9, 3) for k, b in model.items()},
           "share_of_hbm_spec": {k: round(b / med[k] / 1e9 / HBM_SPEC_TBPS, 3) for k, b in model.items()},
           "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default=",".join(CONFIGS), help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
