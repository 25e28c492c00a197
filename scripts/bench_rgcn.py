#!/usr/bin/env python3
"""Measurement (GPU box): the relation-typed aggregation -- ops.spmm_typed (one gather of every neighbour row feeding B slabs) and
ops.spmm_typed_bwd (one walk of the transposed rows) -- against the compositions of existing calls they replace, in one process, for
(R, B) = (8, one-hot), (32, 4), (128, 8) with the 1 / |N_r(i)| weights of R-GCN's mean:

    one-hot composition    R ops.spmm calls on the per-relation restrictions of the graph, each writing its slab of M; backward: R
                           ops.spmm calls on the restrictions of CSR(A^T), beta = 1 from the second on
    basis composition      torch: Xg = X[cols] once, then per basis M_b.index_add_(0, rows, Xg * w[:, b]); backward: per basis
                           dX.index_add_(0, cols, dM[rows, slab b] * w[:, b])   (w = C[etype] * norm, built outside the timed region)
    coefficient gradient   ops.typed_coeff_grad (basis modes), no composition timed
    train_step             RgcnStack([F, F, F]) on every third row

    every kernel: --repeats single calls between two device events after --warmup calls; the median and the range are reported

Byte model, per call, against the 8 TB/s HBM specification (every matrix counted once, although gathered rows come from cache):
    spmm_typed        nnz * (4 F [X row] + 12 [colidx, etype, vals])  +  n * (4 B F [M] + 4 [rowptr])
    spmm_typed_bwd    nnz * (4 S F [dM slabs: S = B, 1 in one-hot mode] + 12)  +  n * (4 F + 4)

One JSON line per configuration: rmat1m_f64 / rmat1m_f128 -- R-MAT 1 M vertices / 10 M listed edges, types uniform over R.  Without
--config the script is a driver: it runs every configuration as a child process of its own under a time limit and stops at the first
one that fails.
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

CONFIGS = {"rmat1m_f64": dict(nodes=1_000_000, edges=10_000_000, feat=64, limit=400),
           "rmat1m_f128": dict(nodes=1_000_000, edges=10_000_000, feat=128, limit=400)}
MODES = ((8, None), (32, 4), (128, 8))
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


def restrictions(torch, rowptr, colidx, etype, norm, R):
    """[(rowptr_r, colidx_r, vals_r)]: the entries of each relation as a CSR of its own over the same rows."""
    n = int(rowptr.numel()) - 1
    rows = torch.repeat_interleave(torch.arange(n, device=rowptr.device), (rowptr[1:] - rowptr[:-1]).long())
    out = []
    for r in range(R):
        keep = etype == r
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=rowptr.device)
        ptr[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=n), 0)
        out.append((ptr.to(torch.int32), colidx[keep].contiguous(), norm[keep].contiguous()))
    return rows, out


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
    g = ops.CsrGraph.from_coo(src, dst, n)
    keep = src != dst
    src, dst = src[keep].contiguous(), dst[keep].contiguous()
    X = ops.uniform_pm1(args.seed + 1, (n, F), device=dev)
    deg = g.rowptr[1:] - g.rowptr[:-1]
    out = {"config": args.config, "nodes": n, "nnz": g.nnz, "feat": F, "max_degree": int(deg.max()), "rows_over_4096": int((deg > 4096).sum()),
           "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0), "cells": {}}
    for R, B in MODES:
        etype = torch.randint(0, R, (int(src.numel()),), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seed + R)).to(torch.int32)
        g.set_edge_type(src, dst, etype, R)
        et, et_t, nv, nv_t = g.entry_type, g.entry_type_t, g.typed_norm, g.typed_norm_t
        slabs = R if B is None else B
        coeff = None if B is None else ops.uniform_pm1(args.seed + 3, (R, B), device=dev)
        M = torch.empty((n, slabs * F), dtype=torch.float32, device=dev)
        dM = ops.uniform_pm1(args.seed + 2, (n, slabs * F), device=dev)
        dX = torch.empty_like(X)
        if B is None:
            _, fwd_r = restrictions(torch, g.rowptr, g.colidx, et, nv, R)
            _, bwd_r = restrictions(torch, g.rowptr_t, g.colidx_t, et_t, nv_t, R)

            def fwd_composed():
                for r, (ptr, col, v) in enumerate(fwd_r):
                    ops.spmm(ptr, col, X, out=M[:, r * F:(r + 1) * F], vals=v)

            def bwd_composed():
                for r, (ptr, col, v) in enumerate(bwd_r):
                    ops.spmm(ptr, col, dM[:, r * F:(r + 1) * F], out=dX, vals=v, beta=1.0 if r else 0.0)
        else:
            rows = torch.repeat_interleave(torch.arange(n, device=dev), deg.long())
            cols = g.colidx.long()
            w = (coeff[et.long()] * nv[:, None]).contiguous()

            def fwd_composed():
                Xg = X[cols]
                M.zero_()
                for b in range(B):
                    M[:, b * F:(b + 1) * F].index_add_(0, rows, Xg * w[:, b:b + 1])

            def bwd_composed():
                dX.zero_()
                for b in range(B):
                    dX.index_add_(0, cols, dM[:, b * F:(b + 1) * F][rows] * w[:, b:b + 1])

        kernels = {"spmm_typed": lambda: ops.spmm_typed(g.rowptr, g.colidx, et, X, R, coeff=coeff, vals=nv, out=M),
                   "fwd_composed": fwd_composed,
                   "spmm_typed_bwd": lambda: ops.spmm_typed_bwd(g.rowptr_t, g.colidx_t, et_t, dM, R, F, coeff=coeff, vals_t=nv_t, out=dX),
                   "bwd_composed": bwd_composed}
        if B is not None:
            kernels["typed_coeff_grad"] = lambda: ops.typed_coeff_grad(g.rowptr, g.colidx, et, dM, X, R, coeff, vals=nv, type_order=g.type_order)
        ms = {k: timed(fn) for k, fn in kernels.items()}
        net = ops.RgcnStack(g, [F, F, F], R, n_bases=B, seed=args.seed + 100, device=dev)
        train_rows = torch.arange(0, n, 3, device=dev, dtype=torch.int32)
        target = (torch.arange(n, device=dev) % F).to(torch.int32)
        ms["rgcn_train_step"] = timed(lambda: net.train_step(X, target, train_rows, 0.0))
        del net
        med = {k: statistics.median(v) for k, v in ms.items()}
        model = {"spmm_typed": g.nnz * (4 * F + 12) + n * (4 * slabs * F + 4),
                 "spmm_typed_bwd": g.nnz * (4 * (1 if B is None else B) * F + 12) + n * (4 * F + 4)}
        out["cells"][f"R{R}_" + ("onehot" if B is None else f"B{B}")] = {
            "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "fwd_composed_over_fused": round(med["fwd_composed"] / med["spmm_typed"], 3),
            "bwd_composed_over_fused": round(med["bwd_composed"] / med["spmm_typed_bwd"], 3),
            "share_of_hbm_spec": {k: round(b / med[k] / 1e9 / HBM_SPEC_TBPS, 3) for k, b in model.items()}}
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
