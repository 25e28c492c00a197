#!/usr/bin/env python3
"""Measurement (MI355X): the cross segment attention calls -- n_seeds query rows per graph over that graph's vertices, the attention
readout's shape -- against the only other route, the CSR attention calls on the [B * n_seeds, n] block CSR of the same batch (query row of
graph g stores every vertex of g; the column side runs on its transpose), in one process, the two alternated call by call:

    forward        ops.segment_cross_attention              vs  ops.attn_aggregate
    backward rows  ops.segment_cross_attention_bwd_rows     vs  ops.attn_aggregate_bwd_rows
    backward cols  ops.segment_cross_attention_bwd_cols     vs  ops.attn_aggregate_bwd_cols

on two batches -- "small": --graphs graphs of 16 .. 64 vertices (seeded uniform); "large": --big-graphs graphs of --big-size -- for
(H, D) = (4, 32) and n_seeds 1 and 8.  Every figure: --repeats single calls between two device events after --warmup calls; the median
and the range.  max_diff: the largest |cross - csr| of each output over the largest |csr|; the run fails at the end if one passes 1e-4.
One JSON line per cell."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, D = 4, 32
SEEDS = (1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--big-graphs", type=int, default=64)
    ap.add_argument("--big-size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    load_package()
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    dev = torch.device("cuda:0")

    def timed(calls):
        """{name: (median, min, max) ms} of the alternated calls"""
        ms = {k: [] for k in calls}
        for it in range(args.warmup + args.repeats):
            for k, f in calls.items():
                a, b = capi.Event(), capi.Event()
                a.record(ops._stream())
                f()
                b.record(ops._stream())
                b.sync()
                if it >= args.warmup:
                    ms[k].append(a.elapsed_ms(b))
        return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}

    gen = torch.Generator().manual_seed(11)
    batches = {"small": torch.randint(16, 65, (args.graphs,), generator=gen), "large": torch.full((args.big_graphs,), args.big_size)}
    worst, F = 0.0, H * D
    for name, sizes in batches.items():
        B, sizes = int(sizes.numel()), sizes.to(dev)
        segptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), sizes.cumsum(0)]).to(torch.int32)
        n = int(segptr[-1])
        graph_of = torch.repeat_interleave(torch.arange(B, device=dev), sizes)
        KV = ops.uniform_pm1(3, (n, 2 * F), device=dev)                 # the readout's layout: K and V of the vertices
        K, V = KV[:, :F], KV[:, F:]
        for S in SEEDS:
            n_q = B * S
            qsegptr = torch.arange(B + 1, dtype=torch.int32, device=dev) * S
            # the block CSR: query row g * S + s stores every vertex of graph g, ascending; its transpose: key j stores the S queries of its graph
            length = torch.repeat_interleave(sizes, S)
            rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), length.cumsum(0)])
            owner = torch.repeat_interleave(torch.arange(n_q, device=dev), length)
            colidx = (torch.arange(int(rowptr[-1]), device=dev) - rowptr[owner] + segptr[:-1].long()[owner // S]).to(torch.int32)
            rowptr = rowptr.to(torch.int32)
            rowptr_t = torch.arange(n + 1, dtype=torch.int32, device=dev) * S
            colidx_t = (graph_of[:, None] * S + torch.arange(S, device=dev)[None, :]).reshape(-1).to(torch.int32)
            del owner
            QG = ops.uniform_pm1(5, (n_q, 2 * F), device=dev)
            Q, G = QG[:, :F], QG[:, F:]
            out = {s: [torch.empty((r, F), device=dev) for r in (n_q, n_q, n, n)] for s in ("cross", "csr")}   # Y, dQ, dK, dV
            st = {}

            def fwd_cross():
                st["s"] = ops.segment_cross_attention(segptr, qsegptr, Q, K, V, H, out=out["cross"][0])

            def fwd_csr():
                st["c"] = ops.attn_aggregate(rowptr, colidx, Q, K, V, H, out=out["csr"][0])

            def rows_cross():
                Y, m, z = st["s"]
                st["sd"] = ops.segment_cross_attention_bwd_rows(segptr, qsegptr, G, Q, K, V, Y, H, m, z, dq_out=out["cross"][1])[1]

            def rows_csr():
                Y, m, z = st["c"]
                st["cd"] = ops.attn_aggregate_bwd_rows(rowptr, colidx, G, Q, K, V, Y, H, m, z, dq_out=out["csr"][1])[1]

            def cols_cross():
                ops.segment_cross_attention_bwd_cols(segptr, qsegptr, G, Q, K, V, H, st["s"][1], st["s"][2], st["sd"], dk_out=out["cross"][2],
                                                     dv_out=out["cross"][3])

            def cols_csr():
                ops.attn_aggregate_bwd_cols(rowptr_t, colidx_t, G, Q, K, V, H, st["c"][1], st["c"][2], st["cd"], dk_out=out["csr"][2],
                                            dv_out=out["csr"][3])

            row = {"batch": name, "graphs": B, "n": n, "n_seeds": S, "H": H, "D": D, "forward_ms": timed({"cross": fwd_cross, "csr": fwd_csr}),
                   "bwd_rows_ms": timed({"cross": rows_cross, "csr": rows_csr}), "bwd_cols_ms": timed({"cross": cols_cross, "csr": cols_csr})}
            row["max_diff"] = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("Y", "dQ", "dK", "dV"), out["cross"], out["csr"])}
            worst = max(worst, *row["max_diff"].values())
            print(json.dumps(row), flush=True)
            del colidx, rowptr, length, colidx_t, rowptr_t
    if worst > 1e-4:
        sys.exit(f"the two sides differ by {worst:.3g} of the largest value")


if __name__ == "__main__":
    main()
