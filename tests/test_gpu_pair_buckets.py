"""The records graph's pair-bucket stage at its LDS capacities.

graph_sets.hip from general_kernel through the pair partition,
pair_reduce_kernel, final_kernel<4096 | 8192> and bucket_widen_kernel to the
generic sort-reduce and assemble2_kernel in SetsJob::finish, on inputs built
(tests/pairs_reference.py) to land on a limit, one below it and one above it:
the pair reduce's 3,584 distinct keys, the merged groups' 8,192 slots, full
bands at bw = 4 and bw = 10, the band/hash and compact/general seams, compact
codes across bucket starts, the look-back over overflowed buckets, split hints
the host has to drop, and the pair lists' two capacities.

Every comparison is exact, against the plain model pair_graph: edges and f64
weight bits, totals, and the pair list's keys and counts; on {read, contig}
pairs and on flagged words.  Every case also asserts, from the launch counts,
the path it took (bucket_widen: two launches per overflowed bucket;
relabel_iota: the relabelled rerun; graph_classify / graph_general: one launch
per attempt): an input that misses its path fails.
"""
import ctypes

import numpy as np
import pytest

import pairs_reference as pr
from karma_amd import _lib, engine

pytestmark = pytest.mark.gpu


def launches(ctx, fn):
    """fn() with every launch counted: ({kernel name: launches}, fn's result)."""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        out = fn()
        return {k: v[1] for k, v in ctx.timing_read(256).items()}, out
    finally:
        ctx.timing(False)


def check_path(n_launch, exp, what):
    attempts = 1 + int(exp.relabel) + int(exp.pair_rerun)
    got = {k: n_launch.get(k, 0) for k in ("bucket_widen", "relabel_iota", "graph_classify", "graph_general",
                                          "graph_bucket_final")}
    want = {"bucket_widen": 2 * len(exp.overflow_buckets), "relabel_iota": int(exp.relabel),
            "graph_classify": attempts, "graph_general": attempts, "graph_bucket_final": attempts}
    assert got == want, (what, got, want)
    assert n_launch.get("bucket_assemble", 0) == (1 if exp.overflow_buckets else 0), what


def check_edges(e, m):
    assert np.array_equal(e.a, m.a) and np.array_equal(e.b, m.b)
    assert np.array_equal(e.shared, m.shared)
    assert np.array_equal(e.weight.view(np.uint64), m.weight.view(np.uint64))
    assert np.array_equal(e.totals, m.totals)


def check_case(rec, n, exp, m):
    ctx = _lib.default_context()
    # {read, contig} pairs and flagged words, every launch counted (one stream)
    for flagged in (False, True):
        r = engine.flag_records(rec) if flagged else rec
        n_launch, e = launches(ctx, lambda: engine.graph_from_records(r, n, ctx=ctx, flagged=flagged))
        check_path(n_launch, exp, "flagged" if flagged else "pairs")
        check_edges(e, m)
    # the pair list itself, as production runs it (general reads on the fork stream)
    p = engine.Pairs.from_records(ctx, rec, n)
    try:
        keys, counts, _ = p.get()
        assert np.array_equal(keys, m.keys) and np.array_equal(counts, m.counts)
    finally:
        p.close()


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_pair_bucket_case(name, monkeypatch):
    rec, n, exp, chunk = pr.case(name)
    if chunk:
        monkeypatch.setenv("KARMA_CHUNK", str(chunk))
    check_case(rec, n, exp, pr.case_model(name))


def test_wide_path_second_attempt_covers_a_chunks_reads():
    """Above 2^21 contigs (records_to_pairs_wide, chunks of 8,192 records, no
    relabelling): a chunk whose reads cover chunk + 7 records at 4.5 pairs per
    record, as in second_attempt_suspect."""
    rec, _, _ = pr.build_second_attempt(True, 8192)
    n = 2_200_000
    m = pr.pair_graph(rec, n)
    assert pr.chunk_pairs(rec, 8192)[1] == 8192 * 9 // 2 + 28
    ctx = _lib.default_context()
    for flagged in (False, True):
        r = engine.flag_records(rec) if flagged else rec
        n_launch, e = launches(ctx, lambda: engine.graph_from_records(r, n, ctx=ctx, flagged=flagged))
        assert (n_launch.get("graph_general", 0), n_launch.get("relabel_iota", 0)) == (2, 0), n_launch
        check_edges(e, m)


class DeviceRecords:
    def __init__(self, ctx, rec):
        self.ctx, self.n = ctx, len(rec)
        self.dev = ctypes.c_void_p()
        rec = np.ascontiguousarray(rec, np.uint32)
        _lib.call("karma_dev_alloc", ctx.h, rec.nbytes, ctypes.byref(self.dev))
        _lib.call("karma_memcpy", ctx.h, self.dev, _lib.ptr(rec), rec.nbytes, 0)

    def close(self):
        _lib.load().karma_dev_free(self.ctx.h, self.dev)


@pytest.mark.parametrize("n", [4096, 1024])
@pytest.mark.parametrize("kind", ["overflow", "big_read"])
def test_split_hints_the_host_drops(kind, n):
    """karma_graph_split_hint when the final kernel's in-bucket counts cannot be
    used: a bucket overflowed (its list is rebuilt and every later list moves), or a
    read of 9 records is merged in afterwards.  split() must then search the
    finished list: bounds inside the overflowed bucket, inside the one after it,
    on and off the bucket grid, at 0 and at n_contigs."""
    rec, _, exp = (pr.build_split_overflow if kind == "overflow" else pr.build_split_big_read)(n)
    m = pr.pair_graph(rec, n)
    ctx = _lib.default_context()
    k = exp.overflow_buckets[0] if exp.overflow_buckets else pr.geometry(n).B // 2
    inside = [16 * k + 1, 16 * k + 9, 16 * k + 15, 16 * (k + 1), 16 * (k + 1) + 7]
    d = DeviceRecords(ctx, rec)
    try:
        for bounds in ([0] + inside + [n], [0, 16, 16 * k, 16 * k + 5, 16 * (k + 1) + 3, 16 * (k + 2), n - 1, n],
                       [0, n], [0, 16 * (k + 1) + 3, n]):
            def run():
                job = engine.Pairs.from_records_begin(ctx, n, d.dev.value, d.n, split_bounds=bounds)
                return job.end()
            n_launch, p = launches(ctx, run)
            try:
                assert n_launch.get("bucket_widen", 0) == 2 * len(exp.overflow_buckets)
                assert n_launch.get("graph_big_pairs", 0) == (1 if kind == "big_read" else 0)
                assert n_launch.get("relabel_iota", 0) == 0
                keys, counts, _ = p.get()
                assert np.array_equal(keys, m.keys) and np.array_equal(counts, m.counts)
                for bd in (bounds, [0, 16 * k + 2, n]):
                    want = np.searchsorted(m.keys, np.array(bd, np.uint64) << np.uint64(32))
                    assert np.array_equal(p.split(bd), want), bd
            finally:
                p.close()
    finally:
        d.close()


def test_deferred_step_merged_overflow_runs_again():
    """One deferred step on the 8,193-pair merged-groups input: the overflow is
    raised by the final kernel itself (the pair reduce succeeded), the step's
    status calls for the slow path and the step runs again synchronously; the
    kept outputs equal the model's.  The status word is not readable from
    outside: the rerun shows in the step counts, its reason in the widen
    launches (the input has no big read, no full pair list, a quiet probe)."""
    from test_gpu_step import Run

    rec, n, exp, _ = pr.case("merged_8193")
    m = pr.case_model("merged_8193")
    r = Run(n, rec)
    try:
        r.ctx.timing(True, "bucket_widen")
        r.ctx.timing_reset()
        r.step(count=False)
        r.build.sync()
        widen = r.ctx.timing_read().get("bucket_widen", (0.0, 0))[1]
        r.ctx.timing(False)
        info = r.build.native.info()
        assert info[[4, 5, 6, 14]].tolist() == [1, 1, 1, 0], info.tolist()
        assert widen == 2 * len(exp.overflow_buckets) == 2
        res = r.step(keep=True)
        check_edges(res["edges"], m)
    finally:
        r.close()
