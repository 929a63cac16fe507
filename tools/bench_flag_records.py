#!/usr/bin/env python3
"""karma_records_flag's sorted kernel against a device-to-device copy of the
same bytes, in one process.

The kernel (csrc/flag.hip, flag_sorted_pairs_kernel) is a pure stream: it reads
8 A bytes of {read, contig} pairs and writes 4 A bytes of KARMA_REC_FLAGGED
words.  A hipMemcpyAsync of 6 A bytes device to device reads and writes the same
12 A bytes in total, so its byte rate is the yardstick: the kernel is where it
should be at >= 0.8 of it.

Both are timed with device events on one stream, alternately, after warm-up
runs: the kernel by the library's per-kernel events (karma_timing_*: the
launch alone, without the call's status readback), the copy by a pair of
events around it.  Prints one JSON line.

Usage: python tools/bench_flag_records.py [--config config3] [--runs 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from karma_amd import _lib, engine  # noqa: E402

# (seed, contigs, fragments, paired): bench.py's workloads
CONFIGS = {"config3": (3, 200_000, 100_000_000, True), "config2": (2, 50_000, 10_000_000, True),
           "tiny": (7, 5_000, 500_000, True)}
HIP_MEMCPY_D2D = 3
KERNEL = "flag_sorted_pairs"


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(CONFIGS))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    seed, n, frags, paired = CONFIGS[args.config]
    rec = engine.synth_records(seed, n, 0, frags, paired)
    A = len(rec)
    reads = int(np.count_nonzero(rec[1:, 0] != rec[:-1, 0])) + 1

    ctx = _lib.Context(0)
    stream = _lib.Stream(ctx)  # a stream whose handle this script knows, for its own events
    ctx.set_stream(stream)
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    d_rec = _lib.DevBuf(ctx, (A, 2), np.uint32)
    d_rec.copy_from(rec)
    d_out = _lib.DevBuf(ctx, (A,), np.uint32)
    d_cp = _lib.DevBuf(ctx, (6 * A,), np.uint8)
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        hip_check(hip.hipEventCreate(ctypes.byref(e)), "hipEventCreate")
    s = ctypes.c_void_p(stream.ptr)

    def kernel_ms():
        ctx.timing_reset()
        got = ctypes.c_int64(0)
        _lib.call("karma_records_flag", ctx.h, ctypes.c_void_p(d_rec.ptr), A, _lib.KARMA_REC_SORTED, 1,
                  ctypes.c_void_p(d_out.ptr), 1, ctypes.byref(got))
        assert got.value == reads, (got.value, reads)
        ms, launches = ctx.timing_read()[KERNEL]
        assert launches == 1
        return ms

    def copy_ms():
        hip_check(hip.hipEventRecord(ev[0], s), "hipEventRecord")
        hip_check(hip.hipMemcpyAsync(ctypes.c_void_p(d_cp.ptr), ctypes.c_void_p(d_rec.ptr), ctypes.c_size_t(6 * A),
                                     HIP_MEMCPY_D2D, s), "hipMemcpyAsync")
        hip_check(hip.hipEventRecord(ev[1], s), "hipEventRecord")
        hip_check(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
        ms = ctypes.c_float(0)
        hip_check(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]), "hipEventElapsedTime")
        return float(ms.value)

    ctx.timing(True, only=KERNEL)
    k, c = [], []
    for i in range(args.warmup + args.runs):
        a, b = kernel_ms(), copy_ms()
        if i >= args.warmup:
            k.append(a)
            c.append(b)
    ctx.timing(False)
    # the words of the last run against the numpy model, on the head and the tail
    m = min(A, 1 << 20)
    head = d_out.view(0, m).numpy()
    tail = d_out.view(A - m, m).numpy()
    assert np.array_equal(head, engine.flag_records(rec[:m]))
    want_tail = engine.flag_records(rec[A - m:])
    if A > m and rec[A - m, 0] == rec[A - m - 1, 0]:
        want_tail[0] &= np.uint32(0x7FFFFFFF)
    assert np.array_equal(tail, want_tail)

    byts = 12 * A
    km, cm = statistics.median(k), statistics.median(c)
    out = {"tool": "bench_flag_records", "config": args.config, "records": A, "reads": reads, "runs": args.runs,
           "warmup": args.warmup, "bytes_moved": byts,
           "kernel_ms": {"median": round(km, 4), "min": round(min(k), 4), "max": round(max(k), 4)},
           "copy_ms": {"median": round(cm, 4), "min": round(min(c), 4), "max": round(max(c), 4)},
           "kernel_GBps": round(byts / km / 1e6, 1), "copy_GBps": round(byts / cm / 1e6, 1),
           "kernel_over_copy_rate": round(cm / km, 3), "tile": list(_lib.flag_tile()),
           "build": _lib.build_info()}
    print(json.dumps(out))
    for e in ev:
        hip.hipEventDestroy(e)
    for b in (d_rec, d_out, d_cp):
        b.close()
    ctx.set_stream(None)
    stream.close()
    ctx.close()


if __name__ == "__main__":
    main()
