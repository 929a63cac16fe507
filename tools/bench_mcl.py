#!/usr/bin/env python3
"""engine.mcl / DeviceAdj.mcl (csrc/mcl.hip) on graphs of the workload's shape:
total time, iterations, the time of an iteration on the fused path and on the
general path, and the latency on a cluster-sized graph.

Inputs are the project's synthetic eq classes through karma_graph_eq and
karma_adj_from_edges (the adjacency karma.py's ReadGraph holds): config3
(200,000 contigs, 100M paired fragments), cluster (1,000 contigs, 500,000
fragments: what karma.py calls MCL on, once per HDBSCAN cluster) and tiny.  No
figure here is a pass condition: there is no earlier implementation to compare
with, and the `mcl` binary is not part of this project.

Every input is measured in a fresh child process (the parent never opens the
GPU), after a warm-up call of both paths on a small graph:
  * wall ms: a host clock around DeviceAdj.mcl, which ends in a device
    synchronisation; `reps` calls of each variant, alternating (one iteration
    only, default, general), reported as median [min, max];
  * per-iteration ms of iterations >= 2: (wall of the variant - wall of the
    one-iteration call) / (iterations - 1), from the medians; what the fused
    kernel has to beat is the general path's figure by more than the spread;
  * kernel ms: the library's per-kernel events over one further call of each
    variant, summed per kernel name (mcl_start, mcl_expand, mcl_iter and the
    sort's radix_hist / radix_scatter / scan, which the general path runs).
The two variants' matrices must be equal bit for bit.  Prints one JSON line per
input.

Usage: python tools/bench_mcl.py [--inputs config3,cluster] [--reps 7] [--resource 4] [--inflation 2.0]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name -> (seed, contigs, fragments)
INPUTS = {"config3": (3, 200_000, 100_000_000), "cluster": (5, 1_000, 500_000), "tiny": (9, 300, 4_000)}
KERNELS = ("mcl_start", "mcl_expand", "mcl_iter", "radix_hist", "radix_scatter", "scan")


def adjacency(name, ctx):
    from karma_amd import consumers, engine

    seed, n, f = INPUTS[name]
    genes = engine.synth_genes(seed, n)
    cls_off, members, counts = engine.synth_eq_classes(seed, n, 0, f, True, genes=genes)
    skip = (np.diff(cls_off) == 1).astype(np.uint8)
    e = engine.graph_from_eq(cls_off, members, counts, skip, n, ctx=ctx)
    return consumers.DeviceAdj.from_edges(n, e.a, e.b, e.weight, ctx=ctx), len(e.a)


def spread(ts):
    return {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3),
            "max": round(max(ts) * 1e3, 3)}


def worker(args):
    from karma_amd import _lib

    ctx = _lib.default_context()
    opts = dict(resource=args.resource, inflation=args.inflation)
    warm, _ = adjacency("tiny", ctx)
    for general in (False, True):  # code objects, clocks
        warm.mcl(general=general, **opts)
    adj, edges = adjacency(args.input, ctx)
    variants = {"one_iteration": dict(max_iter=1), "default": dict(), "general": dict(general=True)}
    results, walls = {}, {k: [] for k in variants}
    for _ in range(args.reps):
        for name, kw in variants.items():
            t0 = time.perf_counter()
            results[name] = adj.mcl(**kw, **opts)
            walls[name].append(time.perf_counter() - t0)
    d, g = results["default"], results["general"]
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(d[:3], g[:3])) and d[3:] == g[3:]
    assert same, "the fused and the general path differ"
    kernels = {}
    for name in ("default", "general"):
        ctx.timing(True)
        ctx.timing_reset()
        adj.mcl(**variants[name], **opts)
        table = ctx.timing_read()
        ctx.timing(False)
        kernels[name] = {k: {"ms": round(table[k][0], 3), "launches": table[k][1]} for k in KERNELS if k in table}
    it = d[3]
    med = {k: statistics.median(v) for k, v in walls.items()}
    later = max(it - 1, 1)
    out = {"input": args.input, "nodes": adj.n, "edges": edges, "resource": args.resource,
           "inflation": args.inflation, "iterations": it, "chaos": d[4], "entries": int(d[0][-1]), "reps": args.reps,
           "wall_ms": {k: spread(v) for k, v in walls.items()},
           "per_iteration_ms_after_the_first": {
               "fused": round((med["default"] - med["one_iteration"]) / later * 1e3, 4),
               "general": round((med["general"] - med["one_iteration"]) / later * 1e3, 4)},
           "kernel_ms": kernels, "paths_equal_bit_for_bit": same}
    if "mcl_iter" in kernels["default"]:
        out["mcl_iter_kernel_ms_per_iteration"] = round(kernels["default"]["mcl_iter"]["ms"] / later, 4)
    gk = kernels["general"]
    out["general_kernel_ms_per_iteration"] = round(
        sum(gk[k]["ms"] for k in ("mcl_expand", "radix_hist", "radix_scatter", "scan") if k in gk) / it, 4)
    out["mcl_expand_kernel_ms_per_iteration"] = round(gk["mcl_expand"]["ms"] / it, 4)
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="config3,cluster")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resource", type=int, default=4)
    ap.add_argument("--inflation", type=float, default=2.0)
    ap.add_argument("--limit", type=int, default=420, help="seconds one input's child process may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--input", choices=sorted(INPUTS))
    args = ap.parse_args(argv)
    if args.worker:
        return worker(args)

    from karma_amd import _lib

    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--input", name, "--reps", str(args.reps),
               "--resource", str(args.resource), "--inflation", str(args.inflation)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            raise RuntimeError(f"worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        out = {"tool": "bench_mcl"}
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
        tile = _lib.mcl_tile()
        out["tile"] = [tile.COLS, tile.LANES4, tile.LANES8, tile.CAND_CAP]
        out["build"] = _lib.build_info()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
