#!/usr/bin/env python3
"""engine.hdbscan (csrc/mst.hip, csrc/hdbscan_tree.cpp) on embeddings of the
workload's shape: per-kernel times, Boruvka rounds, the host tail, and, with
--sklearn, scikit-learn's HDBSCAN on the host as what a user would otherwise
run.

Inputs are Gaussian blobs from a fixed seed: config2 (50,000 x 10, 60 blobs),
config3 (200,000 x 10, 300 blobs: the reference's n_components = 10 at config
3's contig count), m2 (50,000 x 2, 6 blobs) and tiny.  A round of mst_nearest
computes every d2(i, j) again: 3 n^2 m f64 operations, set against the nominal
39.3 T/s DESIGN.md §4.1 uses for profile_knn.  No figure here is a pass
condition; scikit-learn computes its own tree with its own tie order, so that
comparison is of cost, not of results.

Every measurement is a fresh child process (the parent never opens the GPU):
  * kernel ms: the library's per-kernel events, summed per kernel name over one
    karma_mreach_mst call on the device-resident matrix, after a warm-up call
    on the first rows;
  * call wall ms: a second, untimed call;
  * tail ms: karma_hdbscan_tree on the host;
  * sklearn: wall time of HDBSCAN(algorithm=...).fit on the host matrix.
Prints one JSON line per input.

Usage: python tools/bench_hdbscan.py [--inputs config2,config3,m2] [--min-cluster-size 5] [--sklearn auto]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name -> (rows, columns, blobs)
INPUTS = {"config2": (50_000, 10, 60), "config3": (200_000, 10, 300), "m2": (50_000, 2, 6), "tiny": (3_000, 10, 6)}
KERNELS = ("profile_knn_block", "profile_knn_merge", "mst_core", "mst_nearest", "mst_reduce", "mst_hook")
NOMINAL_F64_TOPS = 39.3
WARM_ROWS = 4096


def blobs(name):
    n, m, centres = INPUTS[name]
    rng = np.random.default_rng(12)
    c = 10.0 * rng.normal(size=(centres, m))
    return c[rng.integers(0, centres, n)] + rng.normal(size=(n, m))


def spans(n, a, b):
    """The edges join all n rows (a union-find over them)."""
    up = np.arange(n)

    def find(v):
        while up[v] != v:
            up[v] = up[up[v]]
            v = up[v]
        return v

    for i, j in zip(a.tolist(), b.tolist()):
        ri, rj = find(i), find(j)
        if ri == rj:
            return False
        up[ri] = rj
    return True


def worker_device(args):
    from karma_amd import _lib, engine

    x = blobs(args.input)
    n, m = x.shape
    size = args.min_cluster_size
    ctx = _lib.default_context()
    dev = _lib.DevBuf.from_numpy(ctx, x)
    engine.mreach_mst(x[:min(n, WARM_ROWS)], size, ctx=ctx)  # code objects, clocks
    ctx.timing(True)
    ctx.timing_reset()
    a, b, w, core = engine.mreach_mst(dev, size, ctx=ctx)
    table = ctx.timing_read()
    ctx.timing(False)
    t0 = time.perf_counter()
    a2, b2, w2, _ = engine.mreach_mst(dev, size, ctx=ctx)
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    labels, prob = engine.hdbscan_tree(a, b, w, n, size)
    tail = time.perf_counter() - t0
    ok = (len(a) == n - 1 and bool((a < b).all()) and bool((np.diff(w) >= 0).all()) and spans(n, a, b)
          and np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(w.view(np.uint64), w2.view(np.uint64)))
    assert ok, "not a spanning tree in ascending order, or two calls differ"
    kernels = {k: {"ms": round(table[k][0], 3), "launches": table[k][1]} for k in KERNELS if k in table}
    rounds = kernels["mst_nearest"]["launches"]
    per_round = kernels["mst_nearest"]["ms"] / rounds
    ops = 3.0 * n * n * m
    print(json.dumps({
        "input": args.input, "n": n, "m": m, "min_cluster_size": size, "min_samples": size, "kernels": kernels,
        "kernel_ms_total": round(sum(v["ms"] for v in kernels.values()), 2), "rounds": rounds,
        "rounds_bound": int(np.ceil(np.log2(n))), "mst_nearest_ms_per_round": round(per_round, 3),
        "f64_ops_per_round_model": ops, "f64_Tops_per_s_mean_round": round(ops / per_round / 1e9, 2),
        "nominal_f64_Tops_per_s": NOMINAL_F64_TOPS, "call_wall_ms": round(wall * 1e3, 2),
        "host_tail_ms": round(tail * 1e3, 2), "clusters": int(labels.max() + 1), "noise": int((labels == -1).sum()),
        "spanning_sorted_repeatable": ok}))


def worker_sklearn(args):
    from sklearn.cluster import HDBSCAN

    x = blobs(args.input)
    t0 = time.perf_counter()
    model = HDBSCAN(min_cluster_size=args.min_cluster_size, algorithm=args.sklearn, n_jobs=16).fit(x)
    print(json.dumps({"ms": round((time.perf_counter() - t0) * 1e3, 1), "algorithm": args.sklearn,
                      "clusters": int(model.labels_.max() + 1), "noise": int((model.labels_ == -1).sum()),
                      "threads": os.environ.get("OMP_NUM_THREADS")}))


def child(args, worker, name, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", worker, "--input", name,
           "--min-cluster-size", str(args.min_cluster_size), "--sklearn", args.sklearn or "auto"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError(f"{worker} worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="config2,config3,m2")
    ap.add_argument("--min-cluster-size", type=int, default=5)
    ap.add_argument("--sklearn", choices=["auto", "brute", "kd_tree", "ball_tree"],
                    help="also time scikit-learn's HDBSCAN with this algorithm on the host (brute needs n^2 memory)")
    ap.add_argument("--sklearn-limit", type=int, default=600, help="seconds a host comparison may take")
    ap.add_argument("--worker", choices=["device", "sklearn"])
    ap.add_argument("--input", choices=sorted(INPUTS))
    args = ap.parse_args(argv)
    if args.worker:
        return {"device": worker_device, "sklearn": worker_sklearn}[args.worker](args)

    from karma_amd import _lib

    for name in args.inputs.split(","):
        out = {"tool": "bench_hdbscan"}
        out.update(child(args, "device", name, 900))
        if args.sklearn:
            try:
                out["sklearn_host"] = child(args, "sklearn", name, args.sklearn_limit)
            except (subprocess.TimeoutExpired, RuntimeError) as e:
                out["sklearn_host"] = {"failed": type(e).__name__, "limit_s": args.sklearn_limit}
        out["tile"] = list(_lib.mst_tile())
        out["build"] = _lib.build_info()
        out["note"] = "scikit-learn builds its own tree with its own tie order: a comparison of cost, not of results"
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
