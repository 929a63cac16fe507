#!/usr/bin/env python3
"""engine.umap_spectral (csrc/spectral.hip) on tools/bench_umap.py's inputs:
what the spectral start costs and what it buys.

Per input (config2, config3: Gaussian blobs in the profile's 1088 columns, k =
15, dim = 10), in a fresh child process (the parent never opens the GPU):
  * components of the fuzzy graph and graph_components' wall time;
  * umap_spectral at its defaults on the device graph, after a warm-up call on
    a small graph: wall time (--repeats calls: smallest / median / largest) and,
    from the library's own clocks (karma_spectral_last_ms), labelling, reorder
    and the outer rounds, with the share of the rounds the host spent in the
    small per-component eigenproblems; outer rounds, operator applications,
    components not converged;
  * eigsh: scipy.sparse.linalg.eigsh (which="LA", k = dim + 1, tol = 1e-4) per
    component on 16 host threads -- a cost comparison only, umap-learn's way.
The quality input (bench_umap's tiny: 3,000 rows, 6 blobs) runs the layout from
the spectral and from the random start at the same epoch counts and reports the
silhouette of the true blob labels in each.  Nothing here is a pass condition.
Prints one JSON line per input.

Usage: python tools/bench_spectral.py [--inputs config2,config3,quality] [--repeats 3]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench_umap  # noqa: E402  (the inputs and the helpers)

K, DIM = bench_umap.K, bench_umap.DIM
HOST_THREADS = 16
QUALITY_EPOCHS = (50, 200, 500)


def last_ms():
    from karma_amd import _lib

    ms = (ctypes.c_double * 4)()
    _lib.call("karma_spectral_last_ms", ms)
    return list(ms)


def device_graph(name):
    """(ctx, the fuzzy graph on the device, the blob of every row) of a bench_umap input."""
    from karma_amd import _lib, engine

    n, m, centres = bench_umap.INPUTS[name]
    x = bench_umap.blobs(name)
    which = np.random.default_rng(13)
    which.normal(size=(centres, m))
    labels = which.integers(0, centres, n)  # the draw bench_umap.blobs made
    ctx = _lib.default_context()
    dev = _lib.DevBuf.from_numpy(ctx, x)
    del x
    idx, dist = engine.knn_rows(dev, K, ctx=ctx, out_device=True)
    dev.close()
    return ctx, engine.umap_graph(idx, dist, ctx=ctx, out_device=True), labels


def warm_up(ctx):
    from karma_amd import engine

    rng = np.random.default_rng(1)
    idx, dist = engine.knn_rows(rng.normal(size=(2048, 16)), K, ctx=ctx)
    engine.umap_spectral(engine.umap_graph(idx, dist, ctx=ctx), DIM, 1, ctx=ctx)


def eigsh_per_component(graph, comp):
    """Wall ms of scipy's eigsh on every component with more than dim + 2 vertices, on HOST_THREADS threads."""
    from scipy.sparse import csr_matrix, diags
    from scipy.sparse.linalg import eigsh

    indptr, indices, weights = (g.numpy() for g in graph)
    n = len(indptr) - 1
    a = csr_matrix((weights, indices, indptr), shape=(n, n))
    isd = 1.0 / np.sqrt(np.asarray(a.sum(axis=1)).ravel())
    s = diags(isd) @ a @ diags(isd)
    order = np.argsort(comp, kind="stable")
    bounds = np.flatnonzero(np.r_[True, comp[order][1:] != comp[order][:-1], True])
    parts = [order[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)]
    parts = [rows for rows in parts if len(rows) > DIM + 2]
    blocks = [s[rows][:, rows].tocsr() for rows in parts]

    def one(block):
        eigsh(block, k=DIM + 1, which="LA", tol=1e-4, v0=np.ones(block.shape[0]))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        list(pool.map(one, blocks))
    return (time.perf_counter() - t0) * 1e3, len(blocks)


def silhouette(y, labels):
    """The mean silhouette coefficient (Euclidean), as sklearn.metrics.silhouette_score defines it."""
    n = len(y)
    ids = np.unique(labels)
    sums = np.empty((n, len(ids)))
    for lo in range(0, n, 1024):
        d = np.sqrt(((y[lo:lo + 1024, None, :] - y[None, :, :]) ** 2).sum(axis=2))
        for c, lab in enumerate(ids):
            sums[lo:lo + 1024, c] = d[:, labels == lab].sum(axis=1)
    sizes = np.array([(labels == lab).sum() for lab in ids])
    own = np.searchsorted(ids, labels)
    a = sums[np.arange(n), own] / np.maximum(sizes[own] - 1, 1)
    other = sums / sizes[None, :]
    other[np.arange(n), own] = np.inf
    b = other.min(axis=1)
    s = np.where(sizes[own] > 1, (b - a) / np.maximum(a, b), 0.0)
    return float(s.mean())


def worker_cost(args):
    from karma_amd import engine

    ctx, graph, _ = device_graph(args.input)
    n = graph[0].size - 1
    warm_up(ctx)
    (comp, n_comp), comp_ms = bench_umap.timed(lambda: engine.graph_components(graph, ctx=ctx), args.repeats)
    phases = []

    def solve():
        out = engine.umap_spectral(graph, DIM, 42, ctx=ctx, out_device=True, with_stats=True)
        phases.append(last_ms())
        return out

    (y, st), solve_ms = bench_umap.timed(solve, args.repeats)
    ph = np.median(np.array(phases), axis=0)
    eig_ms, eig_blocks = eigsh_per_component(graph, comp)
    sizes = np.bincount(comp)[np.unique(comp)]
    print(json.dumps({
        "input": args.input, "n": n, "k": K, "dim": DIM, "nnz": int(graph[1].size), "components": n_comp,
        "component_rows": {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max())},
        "components_ms": bench_umap.three(comp_ms), "spectral_ms": bench_umap.three(solve_ms),
        "phase_ms_median": {"labelling": round(ph[0], 2), "reorder": round(ph[1], 2), "rounds": round(ph[2], 2),
                            "host_small_problems": round(ph[3], 2)},
        "host_share_of_rounds": round(float(ph[3] / max(ph[2], 1e-9)), 3),
        "outer_rounds": st.outer_rounds, "operator_applications": st.applications,
        "not_converged": st.not_converged, "tol": 1e-4, "max_outer": 100,
        "eigsh_host_ms": round(eig_ms, 1), "eigsh_components": eig_blocks, "eigsh_threads": HOST_THREADS,
        "finite": bool(np.isfinite(y.numpy()).all())}))


def worker_quality(args):
    from karma_amd import engine

    ctx, graph, labels = device_graph("tiny")
    a, b = engine.umap_ab(1.0, 0.1)
    start = engine.umap_spectral(graph, DIM, 42, ctx=ctx)
    rows = []
    for epochs in QUALITY_EPOCHS:
        spectral = engine.umap_layout(graph, DIM, a, b, epochs, 42, init=start, ctx=ctx)
        random = engine.umap_layout(graph, DIM, a, b, epochs, 42, ctx=ctx)
        rows.append({"epochs": epochs, "silhouette_spectral": round(silhouette(spectral, labels), 4),
                     "silhouette_random": round(silhouette(random, labels), 4)})
    print(json.dumps({"input": "quality", "fixture": "tiny", "n": len(labels), "dim": DIM,
                      "silhouette_of_the_start": round(silhouette(start, labels), 4), "layouts": rows}))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="config2,config3,quality")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds one input may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--input")
    args = ap.parse_args(argv)
    if args.worker:
        return worker_quality(args) if args.input == "quality" else worker_cost(args)

    from karma_amd import _lib

    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--input", name, "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            raise RuntimeError(f"worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        out = {"tool": "bench_spectral"}
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
        out["tile"] = _lib.spectral_tile()
        out["build"] = _lib.build_info()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
