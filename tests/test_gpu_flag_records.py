"""GPU: karma_records_flag ((read, contig) pairs -> KARMA_REC_FLAGGED words on
the device, csrc/flag.hip) against its numpy model engine.flag_records, bit for
bit: words and read count.

  * sorted input at every size around the kernel's lane, wave and block tiles
    (karma_records_flag_tile), with read boundaries placed on and across those
    edges, extreme read ids, and the two errors (read ids decrease; a contig id
    >= 2^31) placed at the same edges;
  * pointers off a 16-byte boundary, host and device on either side, overlap;
  * unsorted input against the model on a stable argsort, around the radix
    sort's 4,096-key tile;
  * the graph of unsorted records three ways (the job's own route, the words
    handed over as FlaggedRecords, the oracle);
  * the product boundary: ReadGraph.from_sam / from_contigs still equal their
    goldens, and the flagged classify -- not the pairs one -- served them
    (karma_classify_launches, a count of launches by record format).
"""
import ctypes
import json
import os

import numpy as np
import pytest

from karma_amd import _lib, contig, engine
from karma_amd.contig import Contig
from karma_amd.read_graph import ReadGraph
from oracle import oracle

pytestmark = pytest.mark.gpu

L, W, T = _lib.flag_tile() if os.path.exists(_lib.LIB_PATH) else (4, 256, 4096)
RADIX_TILE = 4096  # sort.hip: keys per radix tile (tests/test_gpu_consumers_device.py section c)
TOP = (1 << 31) - 1
INGEST = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ingest.json")))


def test_tile_is_what_the_cases_assume():
    assert L >= 1 and W == 64 * L and T % W == 0 and T > W
    assert L * 4 == 16  # one 16-byte store per lane


def reads_records(n, seed, lo=1, hi=7, contig_max=TOP + 1):
    """n records in reads of lo..hi-1 records, read ids rising from a non-zero first id."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(lo, hi, max(n, 1))
    ids = np.repeat(5 + np.cumsum(rng.integers(1, 4, len(runs))), runs)[:n]
    return np.stack([ids, rng.integers(0, contig_max, n)], 1).astype(np.uint32)


def device_words(rec, grouped=True):
    fr = engine.flag_records_device(rec, grouped=grouped)
    try:
        assert fr.n_records == len(rec)
        return fr.to_host(), fr.n_reads
    finally:
        fr.close()


def same_as_model(rec, grouped=True):
    rec = np.asarray(rec, np.uint32).reshape(-1, 2)
    model = engine.flag_records(rec if grouped else rec[np.argsort(rec[:, 0], kind="stable")])
    w, reads = device_words(rec, grouped)
    assert w.dtype == np.uint32 and w.shape == model.shape
    assert np.array_equal(w, model)
    assert reads == int((model >> 31).sum())
    return model


SIZES = [0, 1, 2, 3, L - 1, L, L + 1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 1, 3 * T + L + 1]


@pytest.mark.parametrize("kind", ["reads", "own", "one"])
def test_sorted_sizes(kind):
    for n in SIZES:
        rec = reads_records(n, 100 + n)
        if kind == "own":  # every record its own read
            rec[:, 0] = 3 + np.arange(n)
        elif kind == "one":  # all records in one read
            rec[:, 0] = 77
        model = same_as_model(rec)
        if n and kind == "own":
            assert (model >> 31).all()
        if n and kind == "one":
            assert int((model >> 31).sum()) == 1


@pytest.mark.parametrize("edge", [L, W, T, 2 * T])
def test_read_boundaries_on_the_tile_edges(edge):
    n = 2 * T + W + L + 1
    # a read that starts exactly at the edge: that lane / wave / block's first record is flagged
    rec = reads_records(n, edge)
    rec[:edge, 0] = 7
    rec[edge:, 0] = 9
    model = engine.flag_records(rec)
    assert model[edge] >> 31 == 1 and np.flatnonzero(model >> 31).tolist() == [0, edge]
    same_as_model(rec)
    # the same between reads of 1..6 records
    rec = reads_records(n, edge + 1)
    rec[edge:, 0] += np.uint32(1) if rec[edge, 0] == rec[edge - 1, 0] else np.uint32(0)
    assert engine.flag_records(rec)[edge] >> 31 == 1
    same_as_model(rec)
    # a read that spans the edge: that first record carries no flag
    rec = reads_records(n, edge + 2)
    rec[:, 0] = (np.arange(n) + (1 if edge % 3 == 0 else 0)) // 3
    model = engine.flag_records(rec)
    assert model[edge] >> 31 == 0
    same_as_model(rec)
    rec[edge - 2:edge + 3, 0] = rec[edge - 2, 0]  # five records around it
    rec[edge + 3:, 0] += 1
    assert not (engine.flag_records(rec)[edge - 1:edge + 3] >> 31).any()
    same_as_model(rec)


@pytest.mark.parametrize("rec", [
    [(0x7FFFFFFF, 1), (0x7FFFFFFF, 2), (0xFFFFFFFF, 3), (0xFFFFFFFF, 3)],  # the largest id; top bit only
    [(0, 5), (0, 6), (1, 7)],                                              # a first read id of 0
    [(5, 1), (0x80000005, 2)],                                             # ids that differ only in the top bit
    [(0, TOP), (0, 0), (1, TOP)],                                          # the contig id limit
    [(7, 5)], [(7, 0)], [(3, 4), (3, 9), (3, 4), (3, 0)], [(4, 2), (9, 1), (9, 3)],
])
def test_sorted_read_id_values(rec):
    same_as_model(np.array(rec, np.uint32))


def error_positions(n):
    return [1, L, W, T, n - 1]


def test_sorted_errors_at_the_tile_edges():
    n = 2 * T + 3
    base = reads_records(n, 9, contig_max=100)
    good = reads_records(W + 1, 10, contig_max=100)
    for pos in error_positions(n):
        rec = base.copy()
        rec[pos, 0] = rec[pos - 1, 0] - 1  # one decrease
        assert int((rec[1:, 0] < rec[:-1, 0]).sum()) == 1
        with pytest.raises(ValueError):
            engine.flag_records(rec)
        with pytest.raises(_lib.KarmaError) as ei:
            engine.flag_records_device(rec)
        assert ei.value.code == _lib.KARMA_ERR_UNSORTED, (pos, str(ei.value))
        with pytest.raises(_lib.KarmaError) as eg:
            engine.graph_from_records(rec, 100, grouped=True)
        assert eg.value.code == _lib.KARMA_ERR_UNSORTED
        assert str(ei.value) == str(eg.value)  # the pairs path's own message
        same_as_model(good)  # the context is usable afterwards
        rec = base.copy()
        rec[pos, 1] = TOP  # the largest contig a word holds
        same_as_model(rec)
        for bad in (1 << 31, 0xFFFFFFFF):
            rec = base.copy()
            rec[pos, 1] = bad
            with pytest.raises(_lib.KarmaError) as ei:
                engine.flag_records_device(rec)
            assert ei.value.code == _lib.KARMA_ERR_ARG, (pos, bad, str(ei.value))
            with pytest.raises(_lib.KarmaError) as ei:
                engine.flag_records_device(rec, grouped=False)
            assert ei.value.code == _lib.KARMA_ERR_ARG, (pos, bad, str(ei.value))
            same_as_model(good)


def raw_flag(ctx, src, n, fmt, src_dev, dst, dst_dev):
    reads = ctypes.c_int64(-1)
    _lib.call("karma_records_flag", ctx.h, ctypes.c_void_p(src), n, fmt, src_dev, ctypes.c_void_p(dst), dst_dev,
              ctypes.byref(reads))
    return reads.value


def test_pointers_off_a_16_byte_boundary_and_host_or_device_sides():
    ctx = _lib.default_context()
    n = T + W + 3
    rec = reads_records(n, 21)
    model = engine.flag_records(rec)
    reads = int((model >> 31).sum())
    big = _lib.DevBuf(ctx, (2 * n + 8,), np.uint32)
    out = _lib.DevBuf(ctx, (n + 8,), np.uint32)
    assert big.ptr % 16 == 0 and out.ptr % 16 == 0
    for in_off in (0, 2):  # records at base and base + 8 bytes
        stage = np.zeros(2 * n + 8, np.uint32)
        stage[in_off:in_off + 2 * n] = rec.reshape(-1)
        big.copy_from(stage)
        for out_off in (0, 1, 2, 3):  # out at base, + 4, + 8, + 12 bytes
            out.copy_from(np.full(n + 8, 0xDEADBEEF, np.uint32))
            assert raw_flag(ctx, big.ptr + 4 * in_off, n, _lib.KARMA_REC_SORTED, 1, out.ptr + 4 * out_off, 1) == reads
            got = out.numpy()
            assert np.array_equal(got[out_off:out_off + n], model)
            assert (got[:out_off] == 0xDEADBEEF).all() and (got[out_off + n:] == 0xDEADBEEF).all()
    # host in, device out; device in, host out; both host -- sorted and unsorted
    shuf = rec[np.random.default_rng(5).permutation(n)]
    umodel = engine.flag_records(shuf[np.argsort(shuf[:, 0], kind="stable")])
    for fmt, src, want in ((_lib.KARMA_REC_SORTED, rec, model), (_lib.KARMA_REC_UNSORTED, shuf, umodel)):
        src = np.ascontiguousarray(src)
        big.copy_from(np.r_[src.reshape(-1), np.zeros(8, np.uint32)])
        assert raw_flag(ctx, src.ctypes.data, n, fmt, 0, out.ptr, 1) == reads
        assert np.array_equal(out.numpy()[:n], want)
        for src_ptr, src_dev in ((big.ptr, 1), (src.ctypes.data, 0)):
            host = np.full(n + 2, 0xDEADBEEF, np.uint32)
            assert raw_flag(ctx, src_ptr, n, fmt, src_dev, host.ctypes.data + 4, 0) == reads
            assert np.array_equal(host[1:n + 1], want) and host[0] == host[n + 1] == 0xDEADBEEF
    # overlapping records and out
    for o in (big.ptr, big.ptr + 4 * (2 * n - 1), big.ptr - 4 * (n - 1)):
        with pytest.raises(_lib.KarmaError) as ei:
            raw_flag(ctx, big.ptr, n, _lib.KARMA_REC_SORTED, 1, o, 1)
        assert ei.value.code == _lib.KARMA_ERR_ARG and "overlap" in str(ei.value)
    both = np.zeros(3 * n, np.uint32)
    both[:2 * n] = rec.reshape(-1)
    with pytest.raises(_lib.KarmaError) as ei:
        raw_flag(ctx, both.ctypes.data, n, _lib.KARMA_REC_SORTED, 0, both.ctypes.data + 4 * n, 0)
    assert ei.value.code == _lib.KARMA_ERR_ARG
    # ... and ranges that only touch do not
    assert raw_flag(ctx, both.ctypes.data, n, _lib.KARMA_REC_SORTED, 0, both.ctypes.data + 8 * n, 0) == reads
    assert np.array_equal(both[2 * n:], model)
    big.close()
    out.close()


@pytest.mark.parametrize("n", [1, 2, 1000, RADIX_TILE + 1, 2 * RADIX_TILE + 1])
def test_unsorted_against_the_stable_sort(n):
    rng = np.random.default_rng(n)
    pool = rng.integers(0, 1 << 32, max(1, n // 5), dtype=np.int64)  # all four key bytes; ids shared by many
    rec = np.stack([pool[rng.integers(0, len(pool), n)], rng.integers(0, TOP + 1, n)], 1).astype(np.uint32)
    if n > 2:
        assert len(np.unique(rec[:, 0])) < n and (rec[:, 0] >> 24).max() > 0
    same_as_model(rec, grouped=False)
    rec[:, 0] = 0xFEDCBA98  # one read only: the words keep the input order
    model = same_as_model(rec, grouped=False)
    assert np.array_equal(model & TOP, rec[:, 1]) and int((model >> 31).sum()) == 1


def oracle_edges(rec, n):
    rs = np.asarray(rec, np.int64)
    rs = rs[np.argsort(rs[:, 0], kind="stable")]
    starts = np.flatnonzero(np.r_[True, rs[1:, 0] != rs[:-1, 0]])
    return oracle.graph_groups(np.r_[starts, len(rs)], rs[:, 1], None, None, n, dedup=True)


def same_graph(x, o):
    assert np.array_equal(x.a, o["a"]) and np.array_equal(x.b, o["b"])
    assert np.array_equal(x.shared, o["shared"])
    assert np.array_equal(x.weight.view(np.uint64), o["weight"].view(np.uint64))
    assert np.array_equal(x.totals, o["totals"])


@pytest.mark.parametrize("kind", ["synthetic", "spread", "big_read"])
def test_graph_of_unsorted_records_three_ways(kind):
    n = 5000
    rec = np.ascontiguousarray(engine.synth_records(8, n, 0, 40_000, True)[:60_000])
    assert len(rec) == 60_000
    if kind == "spread":  # ids spread over more than 4 contigs: the general path
        rec[:, 1] = np.random.default_rng(3).permutation(n).astype(np.uint32)[rec[:, 1]]
        ids, first = np.unique(rec[:, 0], return_index=True)
        spans = np.maximum.reduceat(rec[:, 1].astype(np.int64), first) - np.minimum.reduceat(
            rec[:, 1].astype(np.int64), first)
        assert (spans > 4).sum() > len(ids) // 4
    if kind == "big_read":  # one read of more than 8 records
        r0 = int(rec[:, 0].max()) + 1
        big = np.stack([np.full(12, r0), np.random.default_rng(4).integers(0, n, 12)], 1).astype(np.uint32)
        rec = np.concatenate([rec, big])
    shuf = rec[np.random.default_rng(0).permutation(len(rec))]
    o = oracle_edges(shuf, n)
    p0, f0 = _lib.classify_launches()
    same_graph(engine.graph_from_records(shuf, n, grouped=False), o)
    p1, f1 = _lib.classify_launches()
    assert p1 == p0 and f1 > f0  # the flagged classify served the unsorted job
    fr = engine.flag_records_device(shuf, grouped=False)
    assert fr.n_reads == len(np.unique(shuf[:, 0]))
    same_graph(engine.graph_from_records(fr, n, flagged=True), o)
    job = engine.Pairs.from_records_begin(_lib.default_context(), n, fr)
    p = job.end()
    e = p.edges(_lib.KARMA_MODE_READS, n)
    same_graph(e.get(), o)
    e.close()
    p.close()
    assert _lib.classify_launches()[0] == p0
    fr.close()
    same_graph(engine.graph_from_records(rec, n, grouped=True), o)  # the pairs route stays
    assert _lib.classify_launches()[0] > p0


def test_unsorted_job_reports_contig_ids_as_the_pairs_path_does():
    msgs = {}
    for bad in (12, 10 + (1 << 24), TOP, 1 << 31, 0xFFFFFFFF):
        rec = np.array([[3, 1], [0, bad], [3, 2]], np.uint32)
        for grouped in (False, True):
            with pytest.raises(_lib.KarmaError) as ei:
                engine.graph_from_records(rec[np.argsort(rec[:, 0], kind="stable")] if grouped else rec, 10,
                                          grouped=grouped)
            assert ei.value.code == _lib.KARMA_ERR_ARG
            msgs[bad, grouped] = str(ei.value)
        assert msgs[bad, False] == msgs[bad, True] and "n_contigs" in msgs[bad, False]
    ok = np.array([[3, 1], [0, 9], [3, 2]], np.uint32)
    same_graph(engine.graph_from_records(ok, 10, grouped=False), oracle_edges(ok, 10))
    for empty in (np.zeros((0, 2), np.uint32), np.array([[5, 4]], np.uint32)):
        e = engine.graph_from_records(empty, 10, grouped=False)
        assert len(e.a) == 0 and int(e.totals.sum()) == len(empty)


# ---- the product boundary -------------------------------------------------------------------

def dump(g):
    return {"nodes": [str(n) for n in g.nodes()],
            "edges": [[str(a), str(b), float(d["weight"])] for a, b, d in g.edges(data=True)]}


def test_from_sam_and_from_contigs_take_the_flagged_route(golden, monkeypatch):
    calls = {}
    monkeypatch.setattr(_lib, "CALL_TIMES", calls)
    p0, f0 = _lib.classify_launches()
    served = 0
    for name, g in INGEST["sam"].items():
        if "raises" in g["out"]:
            continue
        data = bytes.fromhex(g["hex"])
        before = _lib.classify_launches()[1]
        assert dump(ReadGraph.from_sam(data)) == g["out"]["graph"], name
        kept = ReadGraph.from_sam(data, keep_records=True)
        assert dump(kept) == g["out"]["graph"], name
        rec = contig.load_sam_records(data)[0].records
        model = engine.flag_records(rec[np.argsort(rec[:, 0], kind="stable")])
        assert kept._records.n_records == len(rec) and kept._records.n_reads == int((model >> 31).sum())
        assert np.array_equal(kept._records.to_host(), model), name
        served += _lib.classify_launches()[1] > before
    assert served > 0 and "karma_records_flag" in calls
    for name, case in golden["readset_hand"].items():
        cs = []
        for nm, reads in zip(case["names"], case["readsets"]):
            c = Contig(nm)
            c.load_from_iterator([f"{r}\t0\t{nm}\t1\t60\t*" for r in reads])
            cs.append(c)
        assert dump(ReadGraph.from_contigs(cs)) == case["out"], name
    p1, f1 = _lib.classify_launches()
    assert p1 == p0 and f1 > f0  # no pairs classify ran for any of them
    assert calls["karma_graph_records"][0] > 0
