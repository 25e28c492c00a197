#!/usr/bin/env python3
"""Measurement (MI355X): the dense segment attention calls against the only other route to global attention on a batch of graphs, the
CSR attention calls on the COMPLETE block-diagonal CSR of the same batch, in one process, the two alternated call by call:

    forward        ops.segment_attention                    vs  ops.attn_aggregate
    backward rows  ops.segment_attention_bwd_rows           vs  ops.attn_aggregate_bwd_rows
    backward cols  ops.segment_attention_bwd_cols           vs  ops.attn_aggregate_bwd_cols   (the pattern is its own transpose)

on two batches -- "small": --graphs graphs of 16 .. 64 vertices (seeded uniform); "large": --big-graphs graphs of --big-size -- for
(H, D) = (8, 16), (4, 32), (1, 128).  Every figure: --repeats single calls between two device events after --warmup calls; the median
and the range.  extra_MiB: what each side holds beside Q, K, V, G and its outputs -- segptr on one side, rowptr + colidx + the
workspace the CSR calls ask for on the other.  max_diff: the largest |segment - csr| of each output over the largest |csr|; the run fails at
the end if one passes 1e-4.  One JSON line per cell.

--bf16 measures instead the bf16 calls against the f32 calls (bf16_leg) on the same two batches at (4, 32), (2, 64), (1, 128)."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 16), (4, 32), (1, 128))
BF16_SHAPES = ((4, 32), (2, 64), (1, 128))


def bf16_leg(args, torch, ops, dev, batches, timed):
    """--bf16: gnnx_segment_attn*_bf16_f32 against gnnx_segment_attn*_f32 on the same batches, alternated call by call.  The f32 side gets
    the bf16 operands widened to float32 (the same values), so max_diff is the kernels' own arithmetic alone; each side's backward
    uses its own forward's Y and statistics.  to_bf16_ms: what a caller who holds float32 Q, K, V, G pays to convert them, on its own."""
    for name, sizes in batches.items():
        segptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
        n = int(segptr[-1])
        print(json.dumps({"batch": name, "graphs": int(sizes.numel()), "n": n}), flush=True)
        for H, D in BF16_SHAPES:
            F = H * D
            P32 = ops.uniform_pm1(3, (n, 4 * F), device=dev)
            Ph = torch.empty((n, 4 * F), dtype=torch.bfloat16, device=dev)
            ops.to_bf16(P32, out=Ph)
            Pf = Ph.float()
            mats = {"bf16": [Ph[:, k * F:(k + 1) * F] for k in range(4)], "f32": [Pf[:, k * F:(k + 1) * F] for k in range(4)]}   # Q, K, V, G
            out = {s: [torch.empty((n, F), device=dev) for _ in range(4)] for s in mats}   # Y, dQ, dK, dV
            st = {}

            def fwd(s):
                Q, K, V, _ = mats[s]
                st[s] = ops.segment_attention(segptr, Q, K, V, H, out=out[s][0])

            def rows(s):
                Q, K, V, G = mats[s]
                Y, m, z = st[s]
                st[s + "d"] = ops.segment_attention_bwd_rows(segptr, G, Q, K, V, Y, H, m, z, dq_out=out[s][1])[1]

            def cols(s):
                Q, K, V, G = mats[s]
                ops.segment_attention_bwd_cols(segptr, G, Q, K, V, H, st[s][1], st[s][2], st[s + "d"], dk_out=out[s][2], dv_out=out[s][3])

            both = lambda f: {s: (lambda s=s: f(s)) for s in ("bf16", "f32")}  # noqa: E731
            row = {"batch": name, "H": H, "D": D, "forward_ms": timed(both(fwd)), "bwd_rows_ms": timed(both(rows)),
                   "bwd_cols_ms": timed(both(cols)), "to_bf16_ms": timed({"QKVG": lambda: ops.to_bf16(P32, out=Ph)})["QKVG"]}
            row["max_diff"] = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("Y", "dQ", "dK", "dV"), out["bf16"], out["f32"])}
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--big-graphs", type=int, default=64)
    ap.add_argument("--big-size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bf16", action="store_true", help="the bf16 calls against the f32 calls on the same (bf16-valued) operands instead")
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
    if args.bf16:
        return bf16_leg(args, torch, ops, dev, batches, timed)
    worst = 0.0
    for name, sizes in batches.items():
        segptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
        n = int(segptr[-1])
        # the complete block-diagonal CSR: row i of graph g stores every vertex of g, ascending
        length = torch.repeat_interleave(sizes.to(dev), sizes.to(dev))
        start = torch.repeat_interleave(segptr[:-1].long(), sizes.to(dev))
        rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), length.cumsum(0)])
        nnz = int(rowptr[-1])
        owner = torch.repeat_interleave(torch.arange(n, device=dev), length)
        colidx = (torch.arange(nnz, device=dev) - rowptr[owner] + start[owner]).to(torch.int32)
        del owner
        rowptr = rowptr.to(torch.int32)
        print(json.dumps({"batch": name, "graphs": int(sizes.numel()), "n": n, "nnz": nnz}), flush=True)
        for H, D in SHAPES:
            F = H * D
            P = ops.uniform_pm1(3, (n, 4 * F), device=dev)            # the stack's layout: column slabs of one product
            Q, K, V, G = (P[:, k * F:(k + 1) * F] for k in range(4))
            ws, _ = ops._scratch("gnnx_attn_workspace", n, nnz, H, D, device=dev, tag="attn")
            out = {s: [torch.empty((n, F), device=dev) for _ in range(4)] for s in ("seg", "csr")}   # Y, dQ, dK, dV
            st = {}

            def fwd_seg():
                st["s"] = ops.segment_attention(segptr, Q, K, V, H, out=out["seg"][0])

            def fwd_csr():
                st["c"] = ops.attn_aggregate(rowptr, colidx, Q, K, V, H, out=out["csr"][0])

            def rows_seg():
                Y, m, z = st["s"]
                st["sd"] = ops.segment_attention_bwd_rows(segptr, G, Q, K, V, Y, H, m, z, dq_out=out["seg"][1])[1]

            def rows_csr():
                Y, m, z = st["c"]
                st["cd"] = ops.attn_aggregate_bwd_rows(rowptr, colidx, G, Q, K, V, Y, H, m, z, dq_out=out["csr"][1])[1]

            def cols_seg():
                ops.segment_attention_bwd_cols(segptr, G, Q, K, V, H, st["s"][1], st["s"][2], st["sd"], dk_out=out["seg"][2], dv_out=out["seg"][3])

            def cols_csr():
                ops.attn_aggregate_bwd_cols(rowptr, colidx, G, Q, K, V, H, st["c"][1], st["c"][2], st["cd"], dk_out=out["csr"][2], dv_out=out["csr"][3])

            row = {"batch": name, "H": H, "D": D, "forward_ms": timed({"segment": fwd_seg, "csr": fwd_csr}),
                   "bwd_rows_ms": timed({"segment": rows_seg, "csr": rows_csr}), "bwd_cols_ms": timed({"segment": cols_seg, "csr": cols_csr})}
            row["max_diff"] = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("Y", "dQ", "dK", "dV"), out["seg"], out["csr"])}
            row["extra_MiB"] = {"segment": round(4 * segptr.numel() / 2 ** 20, 3),
                                "csr": round((4 * rowptr.numel() + 4 * colidx.numel() + ws.numel() * ws.element_size()) / 2 ** 20, 3)}
            worst = max(worst, *row["max_diff"].values())
            print(json.dumps(row), flush=True)
        del colidx, rowptr, length, start
    if worst > 1e-4:
        sys.exit(f"the two sides differ by {worst:.3g} of the largest value")


if __name__ == "__main__":
    main()
