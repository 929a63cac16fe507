#!/usr/bin/env python3
"""engine.umap_graph and engine.umap_layout (csrc/umap.hip) on profiles of the
workload's shape: the graph and the layout timed separately, the layout per
epoch, and what a hub costs.

Inputs are Gaussian blobs from a fixed seed in the profile's column count:
config2 (50,000 x 1088, 60 blobs), config3 (200,000 x 1088, 300 blobs) and
tiny; k = 15, dim = 10, umap's default epochs (500 up to 10,000 rows, 200
above), negative_sample_rate 5.  umap-learn is not a dependency and is not
timed: there is nothing to race, and no figure here is a pass condition.

Every input is a fresh child process (the parent never opens the GPU):
  * knn ms: one knn_rows call on the device-resident matrix (the lists stay in
    HBM), for scale only;
  * graph ms: wall time of umap_graph on the device lists, after a warm-up call
    on the first rows; --repeats calls, smallest / median / largest;
  * layout ms: wall time of umap_layout on the device graph (the call waits for
    the last epoch), after a warm-up of two epochs; --repeats calls, the same
    three figures, and the median per epoch;
  * walk: a vertex's row is walked by one thread.  Row lengths (entries) and
    the moves a vertex makes over the run (an entry of weight w fires
    n_epochs * w / wmax times, each with 1 + negative_sample_rate moves),
    largest against median: the hub cost the contract accepts.
Prints one JSON line per input.

Usage: python tools/bench_umap.py [--inputs config2,config3] [--repeats 3]
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
INPUTS = {"config2": (50_000, 1088, 60), "config3": (200_000, 1088, 300), "tiny": (3_000, 1088, 6)}
K, DIM, RATE = 15, 10, 5
WARM_ROWS = 2048


def blobs(name):
    n, m, centres = INPUTS[name]
    rng = np.random.default_rng(13)
    c = rng.normal(size=(centres, m))
    x = np.empty((n, m))
    which = rng.integers(0, centres, n)
    for lo in range(0, n, 8192):  # in blocks: no second n x m temporary
        hi = min(n, lo + 8192)
        x[lo:hi] = c[which[lo:hi]] + 0.3 * rng.normal(size=(hi - lo, m))
    return x


def three(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 2), "median": round(ms[len(ms) // 2], 2), "max": round(ms[-1], 2), "runs": len(ms)}


def timed(fn, repeats):
    out, ms = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def worker(args):
    from karma_amd import _lib, engine

    x = blobs(args.input)
    n, m = x.shape
    epochs = engine.umap_default_epochs(n)
    ctx = _lib.default_context()
    dev = _lib.DevBuf.from_numpy(ctx, x)
    del x
    t0 = time.perf_counter()
    idx, dist = engine.knn_rows(dev, K, ctx=ctx, out_device=True)
    knn_ms = (time.perf_counter() - t0) * 1e3
    dev.close()

    warm = min(n, WARM_ROWS)
    hi, hd = idx.numpy()[:warm], dist.numpy()[:warm]
    hi = np.where(hi < warm, hi, 0).astype(np.int32)  # any valid lists do for a warm-up
    engine.umap_graph(hi, hd, ctx=ctx)
    graph, graph_ms = timed(lambda: engine.umap_graph(idx, dist, ctx=ctx, out_device=True), args.repeats)
    a, b = engine.umap_ab(1.0, 0.1)
    engine.umap_layout(graph, DIM, a, b, 2, 42, negative_sample_rate=RATE, ctx=ctx)
    y, layout_ms = timed(lambda: engine.umap_layout(graph, DIM, a, b, epochs, 42, negative_sample_rate=RATE, ctx=ctx),
                         args.repeats)

    indptr, weights = graph[0].numpy(), graph[2].numpy()
    rows = np.diff(indptr)
    wmax = weights.max()
    fires = np.where(weights >= wmax / epochs, epochs * weights / wmax, 0.0) * (1 + RATE)
    moves = np.add.reduceat(np.append(fires, 0.0), indptr[:-1]) * (rows > 0)
    lay = three(layout_ms)
    print(json.dumps({
        "input": args.input, "n": n, "m": m, "k": K, "dim": DIM, "epochs": epochs, "negative_sample_rate": RATE,
        "nnz": int(indptr[-1]), "knn_ms": round(knn_ms, 1), "graph_ms": three(graph_ms), "layout_ms": lay,
        "layout_ms_per_epoch_median": round(lay["median"] / epochs, 3),
        "row_entries": {"max": int(rows.max()), "median": float(np.median(rows)),
                        "max_over_median": round(float(rows.max() / max(np.median(rows), 1.0)), 2)},
        "vertex_moves": {"max": round(float(moves.max()), 1), "median": round(float(np.median(moves)), 1),
                         "max_over_median": round(float(moves.max() / max(np.median(moves), 1.0)), 2)},
        "finite": bool(np.isfinite(y).all())}))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="config2,config3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds one input may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--input", choices=sorted(INPUTS))
    args = ap.parse_args(argv)
    if args.worker:
        return worker(args)

    from karma_amd import _lib

    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--input", name, "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            raise RuntimeError(f"worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        out = {"tool": "bench_umap"}
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
        out["tile"] = _lib.umap_tile()
        out["build"] = _lib.build_info()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
