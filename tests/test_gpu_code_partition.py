"""The records graph's code-partition path at its limits, against the oracle.

From 57 code buckets on (and whenever KARMA_BIN=0) classify's compact codes
reach the per-bucket histograms through graph_code_partition and
graph_code_reduce: partition_kernel<CodeStream> up to 128 code buckets (path
2: per-flush padded runs, 8,192 codes a flush), code_append_kernel from 129 on
(path 3: one appended run per block and bucket, 12,288 codes a flush), then
code_reduce_kernel through stream_runs.  tests/code_partition_reference.py
builds inputs whose partition blocks have given per-flush, per-bucket
histograms, from the geometry the library reports (karma_graph_code_geometry:
lists per block, blocks, codes per flush; KARMA_PART_RESIDENT makes blocks of
many lists out of few chunks): block items on both sides of one and two
flushes, a flush in one bucket (rank flush - 1 in the packed 16-bit ranks),
counts of 1 (mod 8) and of every residue, buckets and lists and blocks with no
code, 128 lists a block, the append kernel's worst-case regions (7 pending
codes, then 2 (mod 8) new ones, in every bucket: past the staging array's
earlier size from 294 buckets on), directory rows that split a run into 64,
57, 2 and 1 pieces, a wave's 64 pieces on both sides of one stream_runs round,
a relabelled rerun with block histograms, a second reduce group, and a
deferred step followed by a kept one.

Edges, f64 weight bits and totals are compared exactly with
oracle.graph_groups, on {read, contig} pairs and on flagged words.  Every case
asserts the path from the geometry and, from the launch table, that
graph_code_partition and graph_code_reduce ran once per attempt.

The cases stay under 300,000 records, but for two kinds the path cannot give
smaller: 511 to 513 directory rows take as many chunks of 2,048 records, and a
second reduce group takes more than Bc << 18 records (15 M at 57 buckets).
"""
import numpy as np
import pytest

import code_partition_reference as cp
import pairs_reference as pr
from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import ShardedBuild
from oracle import oracle

pytestmark = pytest.mark.gpu


def oracle_graph(rec, n):
    rs = np.asarray(rec, np.int64)
    st = np.flatnonzero(np.r_[True, rs[1:, 0] != rs[:-1, 0]])
    return oracle.graph_groups(np.r_[st, len(rs)], rs[:, 1], None, None, n, dedup=True)


def same(e, o):
    assert np.array_equal(e.a, o["a"]) and np.array_equal(e.b, o["b"])
    assert np.array_equal(e.shared, o["shared"])
    assert np.array_equal(e.weight.view(np.uint64), o["weight"].view(np.uint64))
    assert np.array_equal(e.totals, o["totals"])


def launches(ctx, fn):
    """fn() with every launch counted: ({kernel name: launches}, fn's result)."""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        out = fn()
        return {k: v[1] for k, v in ctx.timing_read(256).items()}, out
    finally:
        ctx.timing(False)


def settle(monkeypatch, knob):
    monkeypatch.setenv("KARMA_CHUNK", str(cp.CHUNK))
    monkeypatch.delenv("KARMA_BIN", raising=False)
    if knob is None:
        monkeypatch.delenv("KARMA_PART_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("KARMA_PART_RESIDENT", str(knob))


def geometry(ctx, n, n_records, flagged=False):
    geo = _lib.code_geometry(ctx, n, n_records, flagged=flagged)
    g = pr.geometry(n)
    assert (geo.Bc, geo.bwc, geo.chunk) == (g.Bc, g.bwc, cp.CHUNK)
    assert geo.path == (_lib.CODE_PATH_APPEND if g.Bc >= cp.APPEND_MIN_BC else _lib.CODE_PATH_PARTITION)
    assert geo.flush == {2: cp.CODE_FILL, 3: cp.APPEND_CAP}[geo.path] and geo.per_cu >= 1
    assert geo.n_chunks == max(1, -(-n_records // cp.CHUNK)) and geo.n_pblk == -(-geo.n_chunks // geo.lpb)
    return geo


def check(ctx, rec, n, attempts=1, relabel=0, formats=(False, True), o=None):
    """Both record formats through the graph, exact against the oracle; the
    code partition and the code reduce ran once per attempt."""
    o = oracle_graph(rec, n) if o is None else o
    for flagged in formats:
        r = engine.flag_records(rec) if flagged else rec
        n_launch, e = launches(ctx, lambda: engine.graph_from_records(r, n, ctx=ctx, flagged=flagged))
        got = {k: n_launch.get(k, 0) for k in ("graph_classify", "graph_code_partition", "graph_code_reduce",
                                               "relabel_iota")}
        assert got == {"graph_classify": attempts, "graph_code_partition": attempts, "graph_code_reduce": attempts,
                       "relabel_iota": relabel}, (flagged, got)
        same(e, o)
    return o


@pytest.mark.parametrize("name", sorted(cp.CASES))
def test_code_partition_case(name, monkeypatch):
    n, chunks, knob = cp.case_geometry(name)
    settle(monkeypatch, knob)
    ctx = _lib.default_context()
    geo = geometry(ctx, n, chunks * cp.CHUNK)
    assert geometry(ctx, n, chunks * cp.CHUNK, flagged=True) == geo
    if knob is not None:  # the knob caps the resident blocks lpb is derived from
        assert geo.lpb == min(cp.MAX_LISTS, -(-chunks // knob))
    rec = cp.case_records(name, geo)  # asserts its own placement for this geometry
    if name.startswith("rows_"):
        rows = sum(len(fl) for fl in cp.placement(rec, n, geo))
        assert rows == chunks == geo.n_pblk and geo.n_cg == 1
        assert cp.reduce_split(rows) == {1: 64, 8: 64, 9: 57, 511: 2, 512: 1, 513: 1}[rows]
    if name.startswith("worst_case"):
        u = cp.usable(geo, n)
        h = cp.placement(rec, n, geo)[0]
        assert cp.staged(h)[1] == cp.staged_bound(geo.flush, u) > (geo.flush + 8 * cp.MAX_BC if u >= 294 else 0)
    # no relabel (build asserts the probe stays quiet) and no full pair list: one attempt
    assert geo.n_cg == 1
    check(ctx, rec, n)


def test_binned_geometry_and_the_knob(monkeypatch):
    """The geometry entry follows the job's own switches: up to 56 buckets the
    binned classify (path 1) unless KARMA_BIN=0; KARMA_PART_RESIDENT lowers the
    lists per block and never raises them; past the compact path no codes."""
    ctx = _lib.default_context()
    settle(monkeypatch, None)
    A = 40 * cp.CHUNK
    assert _lib.code_geometry(ctx, 3584, A).path == _lib.CODE_PATH_BINNED
    monkeypatch.setenv("KARMA_BIN", "0")
    assert _lib.code_geometry(ctx, 3584, A).path == _lib.CODE_PATH_PARTITION
    monkeypatch.delenv("KARMA_BIN")
    free = _lib.code_geometry(ctx, 3648, A)
    assert (free.lpb, free.n_pblk, free.n_chunks) == (1, 40, 40)
    for knob, lpb in ((1, 40), (3, 14), (40, 1), (1 << 20, 1), (0, 1), (-5, 1)):
        monkeypatch.setenv("KARMA_PART_RESIDENT", str(knob))
        g = _lib.code_geometry(ctx, 3648, A)
        assert (g.lpb, g.n_pblk) == (lpb, -(-40 // lpb)), knob
    monkeypatch.setenv("KARMA_PART_RESIDENT", "1")
    assert _lib.code_geometry(ctx, 3648, 300 * cp.CHUNK).lpb == cp.MAX_LISTS
    with pytest.raises(_lib.KarmaError):
        _lib.code_geometry(ctx, (1 << 21) + 1, A)


def test_append_kernel_keeps_two_blocks_per_cu(monkeypatch):
    """code_append_kernel's staging array grew to the proven bound (19,456
    codes, 69 KB of LDS a block): its resident blocks per CU stay at the 2 its
    128 VGPRs allow; partition_kernel<CodeStream> keeps 3."""
    settle(monkeypatch, None)
    ctx = _lib.default_context()
    assert _lib.code_geometry(ctx, 1_600_000, 1 << 20).per_cu == 2
    assert _lib.code_geometry(ctx, 3648, 1 << 20).per_cu == 3


def test_relabelled_rerun_with_block_histograms(monkeypatch):
    """Shuffled contig ids at 129 buckets: the probe calls for the relabelled
    rerun, whose classify counts the block histograms code_append_kernel
    appends by (several lists a block, several blocks)."""
    n, A = 524289, 60 * cp.CHUNK - 77
    settle(monkeypatch, 7)
    ctx = _lib.default_context()
    geo = geometry(ctx, n, A)
    assert (geo.lpb, geo.n_pblk) == (9, 7)
    rec = cp.shuffled_ids(n, A)
    assert pr.relabels(rec, n)
    check(ctx, rec, n, attempts=2, relabel=1)


@pytest.mark.parametrize("flagged", [False, True])
def test_second_reduce_group(flagged, monkeypatch):
    """More than Bc << 18 records at 57 buckets: two reduce groups a bucket,
    over a row count that is no multiple of 2 (group_range's uneven split)."""
    n = 3648
    settle(monkeypatch, None)
    ctx = _lib.default_context()
    Bc = pr.geometry(n).Bc
    # every list but the last holds its chunk's 2,048 codes: a block's rows
    # from its items; the first size past Bc << 18 with an odd row count
    for extra in range(1, 64):
        A = (Bc << cp.CG_SHIFT) + extra * cp.CHUNK + 321
        geo = geometry(ctx, n, A, flagged=flagged)
        items = np.minimum(geo.lpb * cp.CHUNK, A - np.arange(geo.n_pblk) * geo.lpb * cp.CHUNK)
        rows = int((-(-items // geo.flush)).sum())
        if rows % 2:
            break
    assert geo.n_cg == 2 and rows % geo.n_cg != 0, (rows, geo.lpb, geo.n_pblk)
    rng = np.random.default_rng(12)
    rec = np.empty((A, 2), np.uint32)
    rec[:, 0] = np.arange(A, dtype=np.uint32)
    rec[:, 1] = rng.integers(0, n - 3, A, dtype=np.uint32)
    check(ctx, rec, n, formats=(flagged,))


@pytest.mark.parametrize("flagged", [False, True])
def test_deferred_step_then_kept_step(flagged, monkeypatch):
    """code_append_kernel inside the native step: nine blocks of one list at 129
    buckets, a deferred step, then a kept one."""
    name = "rows_9_n524289"
    n, chunks, knob = cp.case_geometry(name)
    settle(monkeypatch, knob)
    ctx = _lib.Context(0)
    rec = cp.case_records(name, geometry(ctx, n, chunks * cp.CHUNK))
    o = oracle_graph(rec, n)
    blob, offs, key_len = engine.synth_contigs(41, n, 30, 2, 0)
    build = ShardedBuild(ctx, SoloComm(), -1, n, 0, n, flagged=flagged)
    store = engine.ContigStore(ctx, blob, offs, key_len)
    dev = _lib.DevBuf.from_numpy(ctx, engine.flag_records(rec) if flagged else rec.view(np.int64).reshape(-1))
    try:
        assert build.native is not None
        assert build.run(store, dev.ptr, len(rec), count=False)["E_local"] is None
        build.sync()
        e_def, deferred = build.native.newest_edges()
        assert deferred
        same(e_def, o)
        res = build.run(store, dev.ptr, len(rec), keep=True)
        same(res["edges"], o)
    finally:
        build.close()
        store.close()
        dev.close()
        ctx.close()
