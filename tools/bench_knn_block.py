#!/usr/bin/env python3
"""The blockwise neighbour lists (csrc/knn_block.hip: kernels profile_knn_block
and profile_knn_merge) on a config's k-mer profile.  Three questions, each
answered in fresh child processes (the parent never opens the GPU), the two
sides of a comparison alternated inside one process:

  carry  what the carried lists cost: karma_knn_block with q = c = the whole
         profile, one block, S = 1, against karma_knn_rows on the same matrix
         (per-kernel events, alternated --reps times per process);
  split  whether the candidate split pays: the first --rows rows of the profile
         as queries against all of it, S = 1 against auto (block + merge
         kernel ms; the two states are compared bit for bit);
  ring   distributed.knn_sharded with --world ranks as threads on this one GPU
         (HostComm: the exchange is staged through host memory), wall time of
         the slowest rank.  A rehearsal of the code path only: no cross-device
         time exists in it.

Prints one JSON line per question.

Usage: python tools/bench_knn_block.py [carry|split|ring ...] [--config config2] [--k 15] [--runs 3] [--reps 3]
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_knn import CONFIGS, WARM_ROWS, device_profile  # noqa: E402

BLOCK, MERGE, ROWS_KERNEL = "profile_knn_block", "profile_knn_merge", "profile_knn"


def timed(ctx, fn):
    """({kernel: ms}, fn's wall ms) of one call."""
    ctx.timing(True)
    ctx.timing_reset()
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    ms = {k: v[0] for k, v in ctx.timing_read(64).items()}
    ctx.timing(False)
    return ms, wall


def worker_carry(args):
    from karma_amd import _lib, engine

    dev = device_profile(args.config)
    ctx = dev.ctx
    n, m = dev.shape
    engine.knn_rows(dev, args.k, 0, min(n, WARM_ROWS), ctx=ctx, out_device=True)  # code objects, clocks
    w = min(n, WARM_ROWS)
    warm = engine.KnnState(ctx, n, args.k)
    warm.update(dev, _lib.DevBuf(ctx, (w, m), np.float64, _ptr=dev.ptr, _owner=dev), 0, cand_split=1)
    warm.close()
    rows_ms, block_ms = [], []
    want = None
    for _ in range(args.reps):
        out = {}
        ms, _ = timed(ctx, lambda: out.update(r=engine.knn_rows(dev, args.k, ctx=ctx, out_device=True)))
        rows_ms.append(ms[ROWS_KERNEL])
        st = engine.KnnState(ctx, n, args.k)
        ms, _ = timed(ctx, lambda: st.update(dev, dev, 0, cand_split=1))
        block_ms.append(ms[BLOCK])
        assert MERGE not in ms
        if want is None:  # the two entries agree bit for bit
            gi, gd = st.finish()
            wi, wd = out["r"][0].numpy(), out["r"][1].numpy()
            want = bool(np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint64), wd.view(np.uint64)))
            assert want
        st.close()
        for b in out["r"]:
            b.close()
    print(json.dumps({"n": n, "m": m, "rows_ms": rows_ms, "block_ms": block_ms, "equal_bits": want}))


def worker_split(args):
    from karma_amd import _lib, engine

    dev = device_profile(args.config)
    ctx = dev.ctx
    n, m = dev.shape
    nq = min(args.rows, n)
    buf = _lib.DevBuf(ctx, (n, m), np.float64, _ptr=dev.ptr, _owner=dev)
    q = buf.view(0, nq * m, shape=(nq, m))
    auto = _lib.knn_block_split(ctx, nq, n, 0)
    forced = args.force_split or auto
    warm = engine.KnnState(ctx, nq, args.k)
    warm.update(q, buf.view(0, min(n, WARM_ROWS) * m, shape=(min(n, WARM_ROWS), m)), 0, cand_split=forced)
    warm.close()
    one, many, states = [], [], {}
    for _ in range(args.reps):
        for S, into in ((1, one), (forced, many)):
            st = engine.KnnState(ctx, nq, args.k)
            ms, wall = timed(ctx, lambda: st.update(q, buf, 0, cand_split=S))
            into.append({"block_ms": ms[BLOCK], "merge_ms": ms.get(MERGE, 0.0), "wall_ms": wall})
            if S not in states:
                states[S] = (st.keys.numpy(), st.idx.numpy())
            st.close()
    same = all(np.array_equal(a, b) for a, b in zip(states[1], states[forced]))
    assert same
    print(json.dumps({"nq": nq, "nc": n, "m": m, "auto_split": auto, "split": forced, "s1": one, "split_runs": many,
                      "equal_bits": bool(same)}))


def worker_ring(args):
    from karma_amd import _lib, engine
    from karma_amd.comm import HostComm
    from karma_amd.distributed import knn_sharded
    from karma_amd.hostgroup import run_ranks

    dev = device_profile(args.config)
    n, m = dev.shape
    whole = engine.knn_rows(dev, args.k, ctx=dev.ctx)
    host = dev.numpy()
    dev.close()
    W = args.world
    bounds = [n * r // W for r in range(W + 1)]

    def rank_fn(group, rank):
        ctx = _lib.Context(0)
        try:
            local = _lib.DevBuf.from_numpy(ctx, host[bounds[rank]:bounds[rank + 1]])
            comm = HostComm(group)
            comm.barrier()
            t0 = time.perf_counter()
            idx, dist = knn_sharded(comm, ctx, local, bounds, args.k)
            wall = (time.perf_counter() - t0) * 1e3
            local.close()
            return idx, dist, wall
        finally:
            ctx.close()

    parts = run_ranks(W, rank_fn)
    gi, gd = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    same = bool(np.array_equal(gi, whole[0]) and np.array_equal(gd.view(np.uint64), whole[1].view(np.uint64)))
    assert same
    print(json.dumps({"n": n, "m": m, "world": W, "rank_wall_ms": [round(p[2], 1) for p in parts],
                      "equal_bits_with_knn_rows": same}))


WORKERS = {"carry": worker_carry, "split": worker_split, "ring": worker_ring}


def child(args, worker, limit=900):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", worker, "--config", args.config, "--k", str(args.k),
           "--reps", str(args.reps), "--rows", str(args.rows), "--world", str(args.world),
           "--force-split", str(args.force_split)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError(f"{worker} worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", help="carry, split, ring (default: all three)")
    ap.add_argument("--config", default="config2", choices=sorted(CONFIGS))
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3, help="fresh processes per question")
    ap.add_argument("--reps", type=int, default=3, help="alternated repetitions inside a process")
    ap.add_argument("--rows", type=int, default=25_000, help="split: query rows")
    ap.add_argument("--world", type=int, default=8, help="ring: ranks")
    ap.add_argument("--force-split", type=int, default=0, help="split: compare S = 1 with this S instead of auto")
    ap.add_argument("--worker", choices=sorted(WORKERS))
    args = ap.parse_args(argv)
    if args.worker:
        return WORKERS[args.worker](args)

    from karma_amd import _lib

    if any(w not in WORKERS for w in args.what):
        ap.error(f"unknown question in {args.what}: choose from {sorted(WORKERS)}")
    for what in args.what or ["carry", "split", "ring"]:
        runs = [child(args, what) for _ in range(1 if what == "ring" else args.runs)]
        out = {"tool": "bench_knn_block", "what": what, "config": args.config, "k": args.k, "runs": len(runs),
               "reps": args.reps}
        if what == "carry":
            a = [x for r in runs for x in r["rows_ms"]]
            b = [x for r in runs for x in r["block_ms"]]
            out.update(n=runs[0]["n"], m=runs[0]["m"], profile_knn_ms=spread(a), profile_knn_block_ms=spread(b),
                       block_over_rows=round(statistics.median(b) / statistics.median(a), 4),
                       equal_bits=all(r["equal_bits"] for r in runs))
        elif what == "split":
            a = [x["block_ms"] + x["merge_ms"] for r in runs for x in r["s1"]]
            b = [x["block_ms"] + x["merge_ms"] for r in runs for x in r["split_runs"]]
            out.update(nq=runs[0]["nq"], nc=runs[0]["nc"], m=runs[0]["m"], auto_split=runs[0]["auto_split"],
                       split=runs[0]["split"], s1_ms=spread(a), split_ms=spread(b),
                       split_merge_ms=spread([x["merge_ms"] for r in runs for x in r["split_runs"]]),
                       split_over_s1=round(statistics.median(b) / statistics.median(a), 4),
                       equal_bits=all(r["equal_bits"] for r in runs))
        else:
            out.update(runs[0])
            out["note"] = "ranks are threads on one GPU and the exchange is staged through host memory: a rehearsal " \
                          "of the code path, no cross-device time exists in it"
        out["tile"] = list(_lib.knn_tile())
        out["build"] = _lib.build_info()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
