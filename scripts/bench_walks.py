#!/usr/bin/env python3
"""Measurement (GPU box): random walks, CsrGraph.random_walk (gnnx_csr_random_walk), one walk per vertex of a
symmetrised R-MAT graph, walk lengths 20 and 80.

    every figure: --repeats single calls after --warmup calls under a host clock, each followed by a device synchronisation inside the
    clock; the median and the range are reported, with walks/s and steps/s (steps actually taken: positions >= 0 behind the start) of
    the median

    walk_L*_p*_q*    g.random_walk(all vertices, L, seed, p, q) at (p, q) = (1, 1), (0.5, 2), (0.25, 4), a fresh seed per call
    fallback_*       for (0.25, 4): the share of second-order steps that exhaust GNNX_WALK_TRIES attempts and take the exact scan,
                     counted by replaying the contract's formula (tests/walk_ref.py) on the first --sample walks of a device result,
                     which it also checks
    torch_L*         the same uniform walk as a user would write it today, a loop of torch ops per step (rowptr[v], torch.rand, a
                     gather), in the same process -- the only baseline there is: the walk has no predecessor in the library
    copy             a device copy of the [n, L + 1] result: the floor of writing it

--compare-stores (the measurement build: make -C gnn.cpp_amd/csrc EXPERIMENTS=1, selected with GNNX_HIP_LIB=exp) times the shipped
kernel, which stages GNNX_WALK_CHUNK positions in LDS, against the variant in which every lane stores each step itself
(GNNX_WALK_DIRECT), alternating the two call by call.

One JSON line per configuration and mode:
    rmat1m    R-MAT 1 M vertices / 10 M edges (20 M entries symmetrised)
    rmat10m   R-MAT 10 M vertices / 99 M edges: the headline graph

Without --config the script is a driver: it runs every configuration as a child process of its own under a time limit, then the store
comparison as another, and stops at the first one that fails.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"rmat1m": dict(nodes=1_000_000, edges=10_000_000, limit=420), "rmat10m": dict(nodes=10_000_000, edges=99_000_000, limit=900)}
LENGTHS = (20, 80)
PQ = ((1.0, 1.0), (0.5, 2.0), (0.25, 4.0))


def driver(args):
    for name in args.configs.split(","):
        for compare in (False, True):
            cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--repeats", str(args.repeats), "--warmup", str(args.warmup),
                   "--sample", str(args.sample)] + (["--compare-stores"] if compare else [])
            env = dict(os.environ, GNNX_HIP_LIB="exp") if compare else dict(os.environ)
            try:
                r = subprocess.run(cmd, timeout=CONFIGS[name]["limit"], env=env)
            except subprocess.TimeoutExpired:
                print(json.dumps({"config": name, "error": "time limit"}), flush=True)
                return 1
            if r.returncode != 0:
                print(json.dumps({"config": name, "error": f"exit status {r.returncode}"}), flush=True)
                return 1
    return 0


def torch_uniform_walk(torch, rowptr, colidx, starts, L):
    """What a user writes without the kernel: per step two rowptr gathers, a draw, a colidx gather and the bookkeeping of ended walks."""
    n = starts.numel()
    walks = torch.full((n, L + 1), -1, dtype=torch.int32, device=starts.device)
    walks[:, 0] = starts
    cur = starts.long()
    alive = torch.ones(n, dtype=torch.bool, device=starts.device)
    for t in range(L):
        b = rowptr[cur].long()
        d = rowptr[cur + 1].long() - b
        alive &= d > 0
        r = (torch.rand(n, device=starts.device) * d).long().clamp(max=torch.clamp(d - 1, min=0))
        nxt = colidx[(b + r).clamp(max=colidx.numel() - 1)].long()
        cur = torch.where(alive, nxt, cur)
        walks[:, t + 1] = torch.where(alive, nxt, torch.full_like(nxt, -1)).to(torch.int32)
    return walks


def fallback_share(walks, rowptr, colidx, seed, p, q):
    """Replays every second-order step of the host walks with the reference's formula: (steps, fallback steps); asserts the device's
    vertex at each."""
    from tests import walk_ref as wr
    thr = wr.thresholds(p, q)
    rows, sets = {}, {}

    def row(v):
        if v not in rows:
            rows[v] = colidx[rowptr[v]:rowptr[v + 1]].tolist()
        return rows[v]

    def row_set(v):
        if v not in sets:
            sets[v] = set(row(v))
        return sets[v]

    steps = fb = 0
    for w, walk in enumerate(walks.tolist()):
        for t in range(1, len(walk) - 1):
            if walk[t + 1] < 0:
                break
            nxt, took, _ = wr.step_ref(seed, w, t, row(walk[t]), walk[t - 1], row_set(walk[t - 1]), thr)
            assert nxt == walk[t + 1], f"walk {w} step {t}: the device went to {walk[t + 1]}, the reference to {nxt}"
            steps += 1
            fb += took
    return steps, fb


def measure(args):
    import torch

    from __graft_entry__ import load_package
    load_package()
    ops = importlib.import_module("gnncpp_amd.ops")
    capi = importlib.import_module("gnncpp_amd.capi")
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    n, e = cfg["nodes"], cfg["edges"]

    def once(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed(fn):
        for _ in range(args.warmup):
            once(fn)
        return [once(fn) for _ in range(args.repeats)]

    def stats(ms, walks=None):
        out = {"ms_median": round(statistics.median(ms), 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)]}
        if walks is not None:
            steps = int((walks[:, 1:] >= 0).sum())
            sec = statistics.median(ms) * 1e-3
            out.update(steps=steps, walks_per_s=round(walks.shape[0] / sec), steps_per_s=round(steps / sec))
        return out

    src, dst = ops.rmat_edges(args.seed, n, e, 0.57, 0.19, 0.19, device=dev)
    g = ops.CsrGraph.from_coo(torch.cat([src, dst]), torch.cat([dst, src]), n, transpose=False, norm=False)   # symmetrised: no dead ends but isolated vertices
    del src, dst
    deg = g.rowptr[1:] - g.rowptr[:-1]
    starts = torch.arange(n, dtype=torch.int32, device=dev)
    out = {"config": args.config, "nodes": n, "edges": e, "nnz": g.nnz, "max_degree": int(deg.max()), "isolated": int((deg == 0).sum()),
           "repeats": args.repeats, "warmup": args.warmup, "device": capi.device_name(0)}
    seeds = iter(range(10 ** 6))                      # a fresh seed per call
    if args.compare_stores:
        assert os.environ.get("GNNX_HIP_LIB") == "exp", "--compare-stores needs the measurement build (GNNX_HIP_LIB=exp)"
        out["mode"] = "compare_stores"
        for L in LENGTHS:
            buf = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
            for p, q in ((1.0, 1.0), (0.5, 2.0)):
                ms = {"staged": [], "direct": []}
                for i in range(args.warmup + args.repeats):
                    for kind in ("staged", "direct"):
                        os.environ.pop("GNNX_WALK_DIRECT", None)
                        if kind == "direct":
                            os.environ["GNNX_WALK_DIRECT"] = "1"
                        seed = 1000 + i
                        t = once(lambda: ops.random_walk(g.rowptr, g.colidx, starts, L, seed, p, q, out=buf))
                        if i >= args.warmup:
                            ms[kind].append(t)
                        if i == 0:
                            ms[kind + "_walks"] = buf.clone()
                os.environ.pop("GNNX_WALK_DIRECT", None)
                assert torch.equal(ms.pop("staged_walks"), ms.pop("direct_walks")), "the two store variants differ"
                out[f"stores_L{L}_p{p:g}_q{q:g}"] = {k: stats(v) for k, v in ms.items()}
            del buf
        print(json.dumps(out), flush=True)
        return 0
    out["mode"] = "walks"
    for L in LENGTHS:
        buf = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
        other = torch.empty_like(buf)
        out[f"copy_L{L}"] = stats(timed(lambda: other.copy_(buf)))
        del other
        for p, q in PQ:
            ms = timed(lambda: ops.random_walk(g.rowptr, g.colidx, starts, L, next(seeds), p, q, out=buf))
            out[f"walk_L{L}_p{p:g}_q{q:g}"] = stats(ms, buf)
        ms = timed(lambda: torch_uniform_walk(torch, g.rowptr, g.colidx, starts, L))
        out[f"torch_L{L}"] = stats(ms, torch_uniform_walk(torch, g.rowptr, g.colidx, starts, L))
        del buf
    # the fallback rate at (0.25, 4), by the reference formula on a sample of walks
    L, p, q, seed = 20, 0.25, 4.0, 4242
    sample = g.random_walk(starts, L, seed, p, q)[:args.sample].cpu()
    rowptr_h, colidx_h = g.rowptr.cpu().numpy(), g.colidx.cpu().numpy()
    steps, fb = fallback_share(sample, rowptr_h, colidx_h, seed, p, q)
    out[f"fallback_L{L}_p{p:g}_q{q:g}"] = {"sampled_walks": int(sample.shape[0]), "second_order_steps": steps, "fallback_steps": fb,
                                         "share": fb / max(steps, 1)}
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="measure this configuration in this process")
    ap.add_argument("--configs", default="rmat1m,rmat10m", help="driver mode: the configurations to run, each in a child process")
    ap.add_argument("--compare-stores", action="store_true", help="staged against direct stores (measurement build)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=2000, help="walks replayed for the fallback rate")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    return measure(args) if args.config else driver(args)


if __name__ == "__main__":
    sys.exit(main())
