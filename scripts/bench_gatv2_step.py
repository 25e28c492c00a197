#!/usr/bin/env python3
"""Measurement (GPU box): the dynamic-attention calls (ops.gatv2_scores, ops.gatv2_scores_bwd) and one Gatv2Stack.train_step on R-MAT
1 M vertices / 10 M edges, dims [128, 128, 128], in ONE process:

    (a) per (heads, head_dim) cell of width 128 -- (1, 128) and (8, 16) -- the forward call, the backward pass on the forward pattern (dL
        and T) and the backward pass on the transposed pattern (entry_map, beta = 1), each against ops.spmm_heads of the same pattern and
        width in the same run: the yardstick, because it gathers the same nnz * 4 H D bytes of rows.  The operands are the two halves of
        one [n, 256] matrix, as Gatv2Stack passes them.
    (b) Gatv2Stack.train_step against GatStack.train_step on the same graph, loss over a tenth of the rows, for heads None and [8, 1].

Every number: --repeats single calls between two device events after --warmup calls; the median and the range are reported.  One JSON
line per cell and per stack pair.  The graph is not relabelled (CsrGraph.attention_map needs ascending rows)."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = ((1, 128), (8, 16))
DIMS = [128, 128, 128]
HEADS = (None, [8, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    from __graft_entry__ import load_package
    load_package()
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    dev = torch.device("cuda:0")
    n, F = args.nodes, DIMS[1]

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
        t = [one_call_ms(fn) for _ in range(args.repeats)]
        return {"median": round(statistics.median(t), 4), "range": [round(min(t), 4), round(max(t), 4)]}

    src, dst = ops.rmat_edges(args.seed, n, args.edges, 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(src, dst, n)
    g.make_plans(args.chunk, 2 * F)
    map_t = g.attention_map()
    deg = g.rowptr[1:] - g.rowptr[:-1]
    deg_t = g.rowptr_t[1:] - g.rowptr_t[:-1]
    base = {"nodes": n, "nnz": g.nnz, "max_degree": int(deg.max()), "max_degree_t": int(deg_t.max()), "repeats": args.repeats,
            "warmup": args.warmup, "device": capi.device_name(0)}

    Hlr = ops.uniform_pm1(args.seed + 1, (n, 2 * F), device=dev)
    Hl, Hr = Hlr[:, :F], Hlr[:, F:]
    a = ops.uniform_pm1(args.seed + 2, (F,), scale=0.25, device=dev)
    dHlr = torch.zeros((n, 2 * F), dtype=torch.float32, device=dev)
    T = torch.empty((n, F), dtype=torch.float32, device=dev)
    Y = torch.empty((n, F), dtype=torch.float32, device=dev)
    for Hh, D in CELLS:
        e = torch.empty((g.nnz, Hh), dtype=torch.float32, device=dev)
        de = ops.uniform_pm1(args.seed + 3, (g.nnz, Hh), scale=1e-3, device=dev)
        vals = ops.uniform_pm1(args.seed + 4, (g.nnz, Hh), device=dev)
        ms = {
            "spmm_heads": timed(lambda: ops.spmm_heads(g.rowptr, g.colidx, Hr, vals, Hh, out=Y)),
            "spmm_heads_t": timed(lambda: ops.spmm_heads(g.rowptr_t, g.colidx_t, Hl, vals, Hh, out=Y)),
            "gatv2_scores": timed(lambda: ops.gatv2_scores(g.rowptr, g.colidx, Hl, Hr, a, Hh, out=e)),
            "gatv2_bwd_rows_with_T": timed(lambda: ops.gatv2_scores_bwd(g.rowptr, g.colidx, de, Hl, Hr, a, Hh, out=dHlr[:, :F], T_out=T)),
            "gatv2_bwd_rows_no_T": timed(lambda: ops.gatv2_scores_bwd(g.rowptr, g.colidx, de, Hl, Hr, a, Hh, out=dHlr[:, :F])),
            "gatv2_bwd_cols_map_beta1": timed(lambda: ops.gatv2_scores_bwd(g.rowptr_t, g.colidx_t, de, Hr, Hl, a, Hh, entry_map=map_t,
                                                                         out=dHlr[:, F:], beta=1.0)),
            "colsum_T": timed(lambda: ops.colsum(T)),
        }
        ratio = {"scores_over_spmm_heads": round(ms["gatv2_scores"]["median"] / ms["spmm_heads"]["median"], 3),
                 "bwd_rows_over_spmm_heads": round(ms["gatv2_bwd_rows_with_T"]["median"] / ms["spmm_heads"]["median"], 3),
                 "bwd_cols_over_spmm_heads_t": round(ms["gatv2_bwd_cols_map_beta1"]["median"] / ms["spmm_heads_t"]["median"], 3)}
        gathered = g.nnz * 4 * F
        print(json.dumps({**base, "heads": Hh, "head_dim": D, "ms": ms, "ratio": ratio,
                          "gathered_row_GB": round(gathered / 1e9, 3),
                          "scores_gather_TBps": round(gathered / ms["gatv2_scores"]["median"] / 1e9, 3)}), flush=True)
        del e, de, vals
    del Hlr, dHlr, T, Y

    X = ops.uniform_pm1(args.seed + 6, (n, DIMS[0]), device=dev)
    target = (torch.arange(n, device=dev) % DIMS[-1]).to(torch.int32)
    rows = torch.arange(0, n, 10, device=dev, dtype=torch.int32)
    for heads in HEADS:
        out = {**base, "dims": DIMS, "heads": heads}
        for name, make in (("GatStack", lambda: ops.GatStack(g, DIMS, seed=args.seed + 100, device=dev, heads=heads)),
                           ("Gatv2Stack", lambda: ops.Gatv2Stack(g, DIMS, seed=args.seed + 100, device=dev, heads=heads)),
                           ("Gatv2Stack_shared", lambda: ops.Gatv2Stack(g, DIMS, seed=args.seed + 100, device=dev, heads=heads, share_weights=True))):
            net = make()
            out[name + "_train_step_ms"] = timed(lambda: net.train_step(X, target, rows, 0.0))
            del net
        out["v2_over_gat"] = round(out["Gatv2Stack_train_step_ms"]["median"] / out["GatStack_train_step_ms"]["median"], 3)
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
