#!/usr/bin/env python3
"""Measurement (MI355X): the fused graph-attention calls against the chains of per-entry calls they replace, in one process, the two
alternated call by call, on R-MAT 1 M vertices / 10 M listed edges as generated, for (H, D) = (1, 128), (8, 8), (8, 16), (4, 32), (8, 32):

    forward     ops.gat_aggregate                      vs  ops.edge_softmax_heads + GatStack._aggregate
    backward    ops.gat_aggregate_bwd_rows + _bwd_cols  vs  the five launches of GatStack._backward_entries (value gradient, softmax
                backward, two gathers through the transpose map, the per-head row sums, the transposed aggregation)
    train_step  GatStack([128, 64, 16], heads=[8, 1]) on every third row, fused=True vs fused=False, and torch.cuda.max_memory_allocated
                of one step each way (after the stack's buffers exist)

Every figure: --repeats single calls between two device events after --warmup calls; the median and the range.  One JSON line per cell.

Byte model of the fused calls, every array counted once (gathered rows come from cache where they can):
    forward    nnz * (4 F [X row] + 8 H [colterm, twice] + 8 [colidx, twice])  +  n * (4 F [Y] + 16 H + 4)
    bwd, rows  nnz * (4 F + 4 H + 4)  +  n * (8 F [G, Y] + 20 H + 4)
    bwd, cols  nnz * (4 F [G row] + 16 H [rowterm, rowmax, rowsum, dot] + 4)  +  n * (8 F [X, dX] + 8 H + 4)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 128), (8, 8), (8, 16), (4, 32), (8, 32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    load_package()
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    dev = torch.device("cuda:0")
    src, dst = ops.rmat_edges(1, args.nodes, args.edges, device=dev)
    g = ops.CsrGraph.from_coo(src, dst, args.nodes)
    g.make_plans(64, 256)
    n, nnz = g.n, g.nnz
    print(json.dumps({"graph": {"n": n, "nnz": nnz, "longest_row": int((g.rowptr[1:] - g.rowptr[:-1]).max()),
                                "longest_col": int((g.rowptr_t[1:] - g.rowptr_t[:-1]).max())}}), flush=True)

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

    for H, D in SHAPES:
        F = H * D
        net = ops.GatStack(g, [F, F], heads=[H])   # the composition's own helpers, one layer of this shape
        Hm = ops.uniform_pm1(3, (n, F), device=dev)
        G = ops.uniform_pm1(4, (n, F), device=dev)
        ER = ops.gemm(Hm, net.A[0], transB=True)
        rt, ct = ER[:, :H], ER[:, H:]
        dER = torch.empty((n, 2 * H), device=dev)
        state = {}

        def fwd_fused():
            state["f"] = ops.gat_aggregate(g.rowptr, g.colidx, Hm, H, rt, ct, 0.2, bias=net.b[0], relu_out=True)

        def fwd_chain():
            alpha = ops.edge_softmax_heads(g.rowptr, g.colidx, H, rowterm=rt, colterm=ct, negative_slope=0.2)
            state["c"] = (alpha, net._aggregate(0, Hm, alpha, bias=net.b[0], relu_out=True))

        def bwd_fused():
            Y, m, z = state["f"]
            _, dot = ops.gat_aggregate_bwd_rows(g.rowptr, g.colidx, G, Hm, Y, H, rt, ct, m, z, 0.2, bias=net.b[0], drowterm_out=dER[:, :H])
            ops.gat_aggregate_bwd_cols(g.rowptr_t, g.colidx_t, G, Hm, H, rt, ct, m, z, dot, 0.2, dcolterm_out=dER[:, H:])

        def bwd_chain():
            net._saved = [(None, Hm, ER, state["c"][0], None)]
            net._backward_entries(0, G, dER)

        row = {"H": H, "D": D, "forward_ms": timed({"fused": fwd_fused, "chain": fwd_chain}),
               "backward_ms": timed({"fused": bwd_fused, "chain": bwd_chain})}
        print(json.dumps(row), flush=True)
        del net, state

    X = ops.uniform_pm1(5, (n, 128), device=dev)
    target = (torch.arange(n, device=dev) % 16).to(torch.int32)
    rows = torch.arange(0, n, 3, device=dev, dtype=torch.int32)
    nets = {k: ops.GatStack(g, [128, 64, 16], heads=[8, 1], fused=(k == "fused")) for k in ("fused", "chain")}
    step = {k: (lambda net=net: net.train_step(X, target, rows, lr=0.01)) for k, net in nets.items()}
    out = {"train_step_ms": timed(step), "max_memory_allocated_MiB": {}}
    for k, f in step.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out["max_memory_allocated_MiB"][k] = [round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), round(base / 2 ** 20, 1)]   # [peak, before]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
