#!/usr/bin/env python3
"""Measurement (GPU box): ops.knn (gnnx_knn_f32) on point clouds and feature rows.

    every figure: --repeats single calls after --warmup calls under a host clock, each followed by a device synchronisation inside the
    clock; the median and the range are reported, with the pair rate (query-candidate pairs per second) of the median and its share of
    the vector-ALU peak at three operations per feature and pair (--peak-tops: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T
    unfused float32 operations per second; the 157 TFLOP/s of the data sheet count a fused multiply-add as two)

    knn          ops.knn(X, k, segptr, exclude_self=True) with the dispatch of the header
    torch        torch.cdist + topk, cloud by cloud (in row blocks where the distance matrix would not fit), in the same process -- the
                 only baseline there is: the call has no predecessor in the library.  Its distances are the ||a||^2 + ||b||^2 - 2ab
                 form: other bits, and no tie rule
    group_G      (the measurement build: make -C gnn.cpp_amd/csrc EXPERIMENTS=1, selected with GNNX_HIP_LIB=exp) the same call with G
                 lanes per query forced (GNNX_KNN_GROUP_LOG2), G = 1 and the dispatch's own choice among them; every forced result is
                 checked to equal the shipped one bit for bit

One JSON line per shape:
    clouds32x1024_f3    32 clouds of 1024 points, n_feat 3, k 20          clouds32x1024_f64   the same with n_feat 64
    cloud16k_f3         one cloud of 16 384 points, n_feat 3, k 16        cloud128k_f3        one cloud of 131 072 points, n_feat 3, k 16
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "clouds32x1024_f3": dict(clouds=32, points=1024, n_feat=3, k=20),
    "clouds32x1024_f64": dict(clouds=32, points=1024, n_feat=64, k=20),
    "cloud16k_f3": dict(clouds=1, points=16384, n_feat=3, k=16),
    "cloud128k_f3": dict(clouds=1, points=131072, n_feat=3, k=16),
}


def torch_knn(torch, X, k, clouds, points, block=8192):
    out = []
    for b in range(clouds):
        C = X[b * points:(b + 1) * points]
        for r0 in range(0, points, block):
            d = torch.cdist(C[r0:r0 + block], C)
            d[torch.arange(min(block, points - r0), device=X.device), torch.arange(r0, min(r0 + block, points), device=X.device)] = float("inf")
            out.append(d.topk(k, dim=1, largest=False).indices + b * points)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tops", type=float, default=78.6, help="unfused float32 vector operations per second, in 1e12")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch

    from __graft_entry__ import load_package
    load_package()
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    dev = torch.device("cuda:0")
    exp = os.environ.get("GNNX_HIP_LIB") == "exp"

    def once(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed(fn):
        for _ in range(args.warmup):
            once(fn)
        return [once(fn) for _ in range(args.repeats)]

    for name in args.shapes.split(","):
        s = SHAPES[name]
        n, F, k = s["clouds"] * s["points"], s["n_feat"], s["k"]
        pairs = s["clouds"] * s["points"] ** 2

        def stats(ms):
            sec = statistics.median(ms) * 1e-3
            return {"ms_median": round(statistics.median(ms), 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)],
                    "pairs_per_s": round(pairs / sec), "share_of_valu_peak": round(3 * F * pairs / sec / (args.peak_tops * 1e12), 4)}

        X = ops.uniform_pm1(args.seed, (n, F), device=dev)
        ptr = torch.arange(s["clouds"] + 1, dtype=torch.int32, device=dev) * s["points"]
        os.environ.pop("GNNX_KNN_GROUP_LOG2", None)
        out = {"shape": name, **s, "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0), "library": "exp" if exp else "product"}
        ref_idx, ref_dist = ops.knn(X, k, segptr=ptr, exclude_self=True)
        out["knn"] = stats(timed(lambda: ops.knn(X, k, segptr=ptr, exclude_self=True)))
        if not exp:
            out["torch"] = stats(timed(lambda: torch_knn(torch, X, k, s["clouds"], s["points"])))
            t_idx = torch_knn(torch, X, k, s["clouds"], s["points"]).to(torch.int32).sort(1).values     # its rounding may pick other rows
            out["torch_rows_with_the_same_set"] = round(float((ref_idx == t_idx).all(1).float().mean()), 4)
        else:
            for gs in range(7):
                os.environ["GNNX_KNN_GROUP_LOG2"] = str(gs)
                idx, dist = ops.knn(X, k, segptr=ptr, exclude_self=True)
                torch.cuda.synchronize()
                assert torch.equal(idx, ref_idx) and torch.equal(dist.view(torch.int32), ref_dist.view(torch.int32)), f"G = {1 << gs} differs"
                out[f"group_{1 << gs}"] = stats(timed(lambda: ops.knn(X, k, segptr=ptr, exclude_self=True)))
            os.environ.pop("GNNX_KNN_GROUP_LOG2", None)
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
