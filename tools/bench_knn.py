#!/usr/bin/env python3
"""karma_knn_rows (csrc/knn.hip, kernel profile_knn) on a config's k-mer
profile, against two yardsticks that compute a LESS EXACT quantity.

The kernel computes every d2(i, j) as the column-ordered sum acc + t * t in
f64 and the k smallest (d2, index) per row, bit for bit what the numpy model
gives: 3 n^2 M f64 operations for n rows and M columns.  The yardsticks are
what a user would otherwise run: a row-blocked torch "Gram trick"
(|x|^2 + |y|^2 - 2 x.y by f64 GEMM, then topk) on the same device matrix, and
scikit-learn's brute-force search on the host.  Both cancel in the Gram form
and break ties arbitrarily; the comparison is of cost, not of results.

Every measurement is a fresh child process (the parent never opens the GPU):
  * kernel ms: the library's per-kernel events around the one launch, after a
    warm-up call on the first rows; median of --runs processes;
  * torch: device events around the whole blocked search, after one warm-up block;
  * sklearn (--sklearn): wall time of fit + kneighbors on the host profile.
Prints one JSON line.

Usage: python tools/bench_knn.py [--config config3] [--k 15] [--runs 5] [--sklearn] [--no-torch]
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

# (seed, contigs, k-mer mode): bench.py's workloads
CONFIGS = {"config3": (3, 200_000, "5p6"), "config2": (2, 50_000, "5p6"), "tiny": (7, 3_000, "5p6")}
KERNEL = "profile_knn"
WARM_ROWS = 4096


def device_profile(config):
    from collections import OrderedDict

    from karma_amd import engine

    seed, n, kmer = CONFIGS[config]
    blob, offs, key_len = engine.synth_contigs(seed, n, 400, 800, 0)

    class Packed(OrderedDict):
        karma_packed = (blob, offs, key_len)

    dev, cols, _ = engine.kmer_profile_device(Packed(), kmer)
    return dev


def model_rows(x, rows, k):
    """The definition on a few query rows (numpy, column by column)."""
    q = x[rows]
    acc = np.zeros((len(rows), len(x)))
    for c in range(x.shape[1]):
        t = q[:, c, None] - x[None, :, c]
        acc = acc + t * t
    idx = np.lexsort((np.broadcast_to(np.arange(len(x)), acc.shape), acc.view(np.uint64)), axis=1)[:, :k]
    return idx.astype(np.int32), np.sqrt(np.take_along_axis(acc, idx, 1))


def worker_knn(args):
    from karma_amd import _lib, engine

    dev = device_profile(args.config)
    ctx = dev.ctx
    n, m = dev.shape
    engine.knn_rows(dev, args.k, 0, min(n, WARM_ROWS), ctx=ctx, out_device=True)  # code object, clocks
    ctx.timing(True, only=KERNEL)
    ctx.timing_reset()
    t0 = time.perf_counter()
    idx, dist = engine.knn_rows(dev, args.k, ctx=ctx, out_device=True)
    wall = time.perf_counter() - t0
    ms, launches = ctx.timing_read()[KERNEL]
    assert launches == 1
    ctx.timing(False)
    out = {"n": n, "m": m, "k": args.k, "kernel_ms": ms, "call_wall_ms": wall * 1e3}
    if args.check:
        rows = np.array([0, n // 2 + 1, n - 1])
        wi, wd = model_rows(dev.numpy(), rows, args.k)
        gi, gd = idx.numpy()[rows], dist.numpy()[rows]
        out["rows_checked_bit_exact"] = bool(np.array_equal(gi, wi) and
                                             np.array_equal(gd.view(np.uint64), wd.view(np.uint64)))
        assert out["rows_checked_bit_exact"]
    print(json.dumps(out))


def worker_torch(args):
    import torch

    dev = device_profile(args.config)
    x = torch.from_dlpack(dev)
    n, m = x.shape
    sq = (x * x).sum(1)
    block = max(1, min(n, (1 << 29) // max(n, 1)))  # a 4 GiB block of f64 distances

    def search(lo, hi):
        d = sq[lo:hi, None] + sq[None, :] - 2.0 * (x[lo:hi] @ x.T)
        return torch.topk(d, args.k, dim=1, largest=False)

    search(0, min(n, block))
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for lo in range(0, n, block):
        search(lo, min(n, lo + block))
    b.record()
    torch.cuda.synchronize()
    print(json.dumps({"n": n, "m": m, "block_rows": block, "ms": a.elapsed_time(b), "dtype": "float64"}))


def worker_sklearn(args):
    from sklearn.neighbors import NearestNeighbors

    x = device_profile(args.config).numpy()
    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=args.k, algorithm="brute").fit(x).kneighbors(x)
    print(json.dumps({"n": x.shape[0], "m": x.shape[1], "ms": (time.perf_counter() - t0) * 1e3,
                      "threads": os.environ.get("OMP_NUM_THREADS")}))


def child(args, worker, *extra, limit=900):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", worker, "--config", args.config, "--k", str(args.k)]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError(f"{worker} worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(CONFIGS))
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn's brute-force search on the host")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--worker", choices=["knn", "torch", "sklearn"])
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args(argv)
    if args.worker:
        return {"knn": worker_knn, "torch": worker_torch, "sklearn": worker_sklearn}[args.worker](args)

    from karma_amd import _lib

    runs = [child(args, "knn", *(["--check"] if i == 0 else [])) for i in range(args.runs)]
    n, m = runs[0]["n"], runs[0]["m"]
    ms = [r["kernel_ms"] for r in runs]
    med = statistics.median(ms)
    ops = 3.0 * n * n * m
    out = {"tool": "bench_knn", "config": args.config, "n": n, "m": m, "k": args.k, "runs": args.runs,
           "kernel_ms": {"median": round(med, 2), "min": round(min(ms), 2), "max": round(max(ms), 2)},
           "call_wall_ms_median": round(statistics.median(r["call_wall_ms"] for r in runs), 2),
           "f64_ops_model": ops, "f64_Tops_per_s": round(ops / med / 1e9, 2),
           "rows_checked_bit_exact": runs[0].get("rows_checked_bit_exact"),
           "tile": list(_lib.knn_tile()), "build": _lib.build_info()}
    if not args.no_torch:
        t = child(args, "torch")
        out["torch_gram_ms"] = round(t["ms"], 2)
        out["torch_gram_block_rows"] = t["block_rows"]
        out["kernel_over_torch_gram_time"] = round(med / t["ms"], 2)
    if args.sklearn:
        s = child(args, "sklearn", limit=1700)
        out["sklearn_brute_host_ms"] = round(s["ms"], 1)
        out["sklearn_threads"] = s["threads"]
    out["note"] = "yardsticks compute the cancelling Gram form with arbitrary ties: a comparison of cost, not of results"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
