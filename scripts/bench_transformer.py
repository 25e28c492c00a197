#!/usr/bin/env python3
"""Measurement (MI355X): the dot-product attention calls against what they replace, in one process, the two alternated call by call, on
R-MAT 1 M vertices / 10 M listed edges as generated, for (H, D) = (8, 8), (8, 16), (4, 32), (1, 128), with and without edge rows E:

    without E   forward   ops.attn_aggregate                          vs  sddmm_heads (Q pre-scaled) + edge_softmax_heads + spmm_heads
                backward  attn_aggregate_bwd_rows + _bwd_cols         vs  sddmm_heads (dalpha), edge_softmax_heads_bwd, spmm_heads (dQ), two gathers
                                                                          through the transpose map, two spmm_heads on CSR(A^T) (dK, dV)
    with E      forward / backward as above                            vs  the torch composition: K[c] + E[e] and V[c] + E[e] as [nnz, F] arrays, a
                                                                          per-entry dot, the chain's softmax, index_add_ (autograd for the backward)

Every figure: --repeats single calls between two device events after --warmup calls; the median and the range.  In the TIMED fused
backward the [nnz, F] dE is a zeroed array made once outside the timing, as TransformerStack holds it, while autograd allocates its
gradients inside the timed call.  peak_MiB: what torch.cuda.max_memory_allocated rises above the operands during one forward + backward
each way, every output and gradient of either side allocated inside the window (the fused dE and torch's e.grad alike).  max_diff: the
largest |fused - other| of each output over the largest |other|, at the timed size; the run fails at the end if one passes 1e-4.
One JSON line per cell."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 8), (8, 16), (4, 32), (1, 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=30)
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
    n, nnz = g.n, g.nnz
    map_t = g.attention_map()
    rows_e = torch.repeat_interleave(torch.arange(n, device=dev), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols_e = g.colidx.long()
    eidx = torch.arange(nnz, device=dev, dtype=torch.int32)          # forward pattern: e_p = p;  transposed pattern: through the map
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

    def peak(f):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    worst, leaves = 0.0, None
    for H, D in SHAPES:
        F, scale = H * D, D ** -0.5
        P = ops.uniform_pm1(3, (n, 4 * F), device=dev)                # the stack's layout: four column slabs of one product
        Q, K, V, G = (P[:, k * F:(k + 1) * F] for k in range(4))
        for edge in (False, True):
            E = ops.uniform_pm1(4, (nnz, F), device=dev) if edge else None
            st = {}

            def fwd_fused():
                st["f"] = ops.attn_aggregate(g.rowptr, g.colidx, Q, K, V, H, E=E, eidx=eidx if edge else None)

            def bwd_fused():
                Y, m, z = st["f"]
                dQ, dot, dE = ops.attn_aggregate_bwd_rows(g.rowptr, g.colidx, G, Q, K, V, Y, H, m, z, E=E, eidx=eidx if edge else None,
                                                          de_out=st.get("dE"))
                dK, dV = ops.attn_aggregate_bwd_cols(g.rowptr_t, g.colidx_t, G, Q, K, V, H, m, z, dot, E=E, eidx_t=map_t if edge else None)
                st["fo"] = [Y, dQ, dK, dV, dE]

            if not edge:
                Qs = (Q * scale).contiguous()

                def fwd_other():
                    s = ops.sddmm_heads(g.rowptr, g.colidx, Qs, K, H)
                    alpha = ops.edge_softmax_heads(g.rowptr, g.colidx, H, scores=s)
                    st["c"] = (s, alpha, ops.spmm_heads(g.rowptr, g.colidx, V, alpha, H))

                def bwd_other():
                    s, alpha, Y = st["c"]
                    dalpha = ops.sddmm_heads(g.rowptr, g.colidx, G, V, H)
                    ds, _ = ops.edge_softmax_heads_bwd(g.rowptr, g.colidx, H, alpha, dalpha, scores=s)
                    dQ = ops.spmm_heads(g.rowptr, g.colidx, K, ds, H)                                   # dQ / scale
                    dK = ops.spmm_heads(g.rowptr_t, g.colidx_t, Qs, ops.gather_rows(ds, map_t), H)
                    dV = ops.spmm_heads(g.rowptr_t, g.colidx_t, G, ops.gather_rows(alpha, map_t), H)
                    st["oo"] = [Y, dQ, dK, dV, None]
            else:
                st["dE"] = torch.zeros((nnz, F), device=dev)
                leaves = [t.detach().clone().requires_grad_(True) for t in (Q, K, V, E)]

                def fwd_other():
                    q, k, v, e = leaves
                    kp, vp = k[cols_e] + e, v[cols_e] + e
                    s = (q[rows_e] * kp).view(nnz, H, D).sum(2) * scale
                    m = torch.full((n, H), -float("inf"), device=dev).scatter_reduce(0, rows_e[:, None].expand(-1, H), s.detach(), "amax")
                    x = torch.exp(s - m[rows_e])
                    alpha = x / torch.zeros((n, H), device=dev).index_add_(0, rows_e, x)[rows_e]
                    st["c"] = torch.zeros((n, F), device=dev).index_add_(0, rows_e, alpha.repeat_interleave(D, 1) * vp)

                def bwd_other():
                    for t in leaves:
                        t.grad = None
                    st["c"].backward(G, retain_graph=True)
                    st["oo"] = [st["c"].detach()] + [t.grad for t in leaves]

            row = {"H": H, "D": D, "E": edge, "other": "torch" if edge else "chain",
                   "forward_ms": timed({"fused": fwd_fused, "other": fwd_other}), "backward_ms": timed({"fused": bwd_fused, "other": bwd_other})}
            if not edge:
                st["oo"][1] = st["oo"][1] * scale
            row["max_diff"] = {k: float((a - b).abs().max() / b.abs().max())
                               for k, a, b in zip(("Y", "dQ", "dK", "dV", "dE"), st["fo"], st["oo"]) if b is not None}
            worst = max(worst, *row["max_diff"].values())
            # the peaks: nothing but the operands is held, so that each side allocates every output and gradient inside the window
            st.clear()
            for t in leaves or ():
                t.grad = None
            row["peak_MiB"] = {"fused": peak(lambda: (fwd_fused(), bwd_fused()))}
            st.clear()
            row["peak_MiB"]["other"] = peak(lambda: (fwd_other(), bwd_other()))
            print(json.dumps(row), flush=True)
            del st, E
            leaves = None
    if worst > 1e-4:
        sys.exit(f"the two sides differ by {worst:.3g} of the largest value")


if __name__ == "__main__":
    main()
