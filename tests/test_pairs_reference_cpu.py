"""tests/pairs_reference.py without a GPU: the model equals the oracle bit for
bit, and every builder's input meets the condition it was built for, counted
with the model alone (distinct hash pairs per bucket, nonzero band slots, pairs
per chunk, relabel-probe windows on wide reads, pairs per flush group)."""
import numpy as np
import pytest

import pairs_reference as pr
from oracle import oracle


def check_model(rec, n):
    rec = np.asarray(rec, np.int64).reshape(-1, 2)
    m = pr.pair_graph(rec, n)
    o = oracle.graph_groups(pr.read_bounds(rec), rec[:, 1], None, None, n, dedup=True)
    assert np.array_equal(m.a, o["a"]) and np.array_equal(m.b, o["b"])
    assert np.array_equal(m.shared, o["shared"])
    assert np.array_equal(m.weight.view(np.uint64), o["weight"].view(np.uint64))
    assert np.array_equal(m.totals, o["totals"])
    # the list: strictly rising keys, the diagonal holds the totals, the rest the edges
    assert np.all(m.keys[1:] > m.keys[:-1]) and np.all(m.counts > 0)
    a, b = m.keys >> np.uint64(32), m.keys & np.uint64(0xFFFFFFFF)
    assert np.all(a <= b)
    assert np.array_equal(m.counts[a == b], m.totals[m.totals > 0])
    assert np.array_equal(m.counts[a < b], m.shared)
    return m


def test_model_equals_oracle_on_random_inputs():
    rng = np.random.default_rng(17)
    for it in range(300):
        n = int(rng.choice([1, 2, 5, 17, 64, 300]))
        rows, rid = [], 0
        for _ in range(int(rng.integers(0, 40))):
            rid += int(rng.integers(1, 3))  # read ids rise, with holes
            lo = int(rng.integers(0, n))
            width = int(rng.choice([1, 4, 12, n]))
            for c in rng.integers(lo, min(n, lo + width), int(rng.choice([1, 1, 2, 2, 3, 5, 8, 9, 13]))):
                rows.append((rid, int(c)))
        check_model(np.array(rows, np.int64).reshape(-1, 2), n)


def test_model_equals_oracle_on_hand_cases():
    m = check_model(np.zeros((0, 2), np.int64), 7)
    assert len(m.keys) == 0 and m.totals.tolist() == [0] * 7
    m = check_model([(3, 2), (3, 5)], 6)  # one read
    assert m.keys.tolist() == [2 << 32 | 2, 2 << 32 | 5, 5 << 32 | 5] and m.counts.tolist() == [1, 1, 1]
    assert m.weight.tolist() == [1.0]
    m = check_model([(0, 4), (0, 4), (0, 1), (0, 4), (1, 1), (1, 1)], 5)  # duplicate records
    assert m.keys.tolist() == [1 << 32 | 1, 1 << 32 | 4, 4 << 32 | 4] and m.counts.tolist() == [2, 1, 1]
    assert m.weight.tolist() == [(1 / 2 + 1 / 1) / 2]
    m = check_model([(9, 3)] * 4, 4)  # a read of one contig
    assert m.keys.tolist() == [3 << 32 | 3] and len(m.a) == 0 and m.totals.tolist() == [0, 0, 0, 1]
    big = [(0, c) for c in range(0, 27, 3)] + [(1, c % 11) for c in range(40)] + [(2, 3), (2, 30)]  # 9 and 40 records
    check_model(big, 31)


def test_geometry_restates_make_geo():
    g = pr.geometry(4096)
    assert (g.bw, g.bbits, g.B, g.dbits, g.bwc, g.Bc, g.n_pg) == (4, 12, 256, 3, 6, 64, 1)
    g = pr.geometry(1024)
    assert (g.bw, g.B, g.n_pg) == (4, 64, 4)
    g = pr.geometry(16)
    assert (g.bw, g.bbits, g.B, g.n_pg) == (4, 4, 1, 256)
    g = pr.geometry(2032)
    assert (g.B, g.n_pg) == (127, 3)
    assert pr.geometry(2033).n_pg == 1
    g = pr.geometry(20_000)
    assert (g.bw, g.B, g.bwc) == (7, 157, 9)
    g = pr.geometry(262_160)
    assert (g.bw, g.bbits, g.B, g.dbits, g.bwc, g.Bc) == (10, 19, 257, 3, 12, 65)
    assert pr.geometry(4090).B == 256


def test_probe_model_on_hand_windows():
    # 512 records: a probe every 2; all reads (c, c + 9): every window's first whole read is wide
    wide = np.stack([np.repeat(np.arange(256), 2), np.tile([0, 9], 256)], 1)
    assert pr.probe_wide_windows(wide, 10) == (512 - 32) // 2 + 1
    assert pr.probe_wide_windows(wide, 9) == 0  # contig out of range: not counted
    narrow = np.stack([np.repeat(np.arange(256), 2), np.tile([0, 3], 256)], 1)
    assert pr.probe_wide_windows(narrow, 10) == 0
    assert pr.probe_wide_windows(wide[:30], 10) == 0  # no whole window


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_builder_meets_its_condition(name):
    rec, n, exp, chunk = pr.case(name)
    chunk = chunk or pr.CHUNK
    g = pr.geometry(n)
    m = pr.case_model(name)
    assert rec.dtype == np.uint32 and rec[:, 1].max() < n
    assert np.all(np.diff(rec[:, 0].astype(np.int64)) >= 0) and len(rec) % chunk == 0
    assert pr.big_reads(rec) == 0
    # the relabel probe: quiet unless the case is about it
    windows = pr.probe_wide_windows(rec, n)
    assert (windows > 32) == exp.relabel, windows
    if not exp.relabel:
        assert windows == 0
    # pairs per chunk against pcap: the rerun happens exactly when a chunk is above it
    cp = pr.chunk_pairs(rec, chunk)
    assert (max(cp) > chunk // 8) == exp.pair_rerun, max(cp)
    hp = pr.hash_pairs_per_bucket(rec, n)
    if not exp.relabel:
        if g.n_pg == 1 or exp.pair_rerun:
            # one flush group per bucket: the pair reduce sees all of a bucket's keys
            assert sorted(b for b, k in hp.items() if k > pr.HASH_R_FILL) == exp.overflow_buckets
        else:
            # several groups: each stays within the pair reduce, the merge alone overflows
            for lo, hi in pr.flush_groups(rec, n, chunk):
                assert max(pr.hash_pairs_per_bucket(rec, n, lo, hi).values()) <= pr.HASH_R_FILL
            assert sorted(b for b, k in hp.items() if k > pr.HASH_F) == exp.overflow_buckets
    # the case's own figure
    kind, args = pr.CASES[name][0].__name__, pr.CASES[name][1]
    if kind == "build_pair_reduce_fill":
        assert hp == {128: args[0]}
        rep = args[1] if len(args) > 1 else 1
        sel = (m.keys >> np.uint64(32 + 4) == 128) & ((m.keys & np.uint64(0xFFFFFFFF)) - (m.keys >> np.uint64(32)) >= 8)
        assert sel.sum() == args[0] and np.all(m.counts[sel] == rep)
    elif kind == "build_merged_groups":
        assert hp == {pr.MERGED_BUCKET: args[0]}
        assert len(pr.flush_groups(rec, n)) == 4
    elif name == "merged_same_lists":
        assert hp == {pr.MERGED_BUCKET: 2000}
        groups = pr.flush_groups(rec, n)
        assert len(groups) == 4
        for lo, hi in groups:
            assert pr.hash_pairs_per_bucket(rec, n, lo, hi) == {pr.MERGED_BUCKET: 2000}
        sel = (m.keys & np.uint64(0xFFFFFFFF)) - (m.keys >> np.uint64(32)) >= 8
        assert sel.sum() == 2000 and np.all(m.counts[sel] == 4)
    elif name == "merged_one_bucket":
        assert len(m.keys) == 16 * 17 // 2 and len(pr.flush_groups(rec, n)) == 1 and g.n_pg == 256
    elif kind == "build_band_small":
        base = args[1] << 4
        want = sum(1 for a in range(base, min(base + 16, n)) for d in range(8) if a + d < n)
        assert pr.band_slots(rec, n, args[1]) == want and (want == 128) == (args[1] == 0)
        assert hp.get(args[1], 0) == sum(1 for a in range(base, min(base + 16, n)) for d in (8, 9) if a + d < n)
    elif name == "band_full_bw10":
        assert pr.band_slots(rec, n, 128) == pr.BAND and hp == {128: pr.HASH_R_FILL}
        assert int((m.keys >> np.uint64(32 + 10) == 128).sum()) == 11_776
    elif kind == "build_compact_edges":
        k = exp.overflow_buckets[0] if exp.overflow_buckets else (g.B // 2) & ~3
        assert (k << g.bw) % (1 << g.bwc) == 0 and ((k + 1) << g.bw) % (1 << g.bwc) != 0
        if args[1]:
            assert hp == {k: pr.HASH_R_FILL + 1, k + 1: pr.HASH_R_FILL + 1}
        else:
            assert hp == {}
        # compact reads reach across both starts: pairs (start - i, start + j) exist
        for start in (k << g.bw, (k + 1) << g.bw):
            for i in (1, 2, 3):
                assert np.uint64((start - i) << 32 | start) in m.keys
    elif kind == "build_lookback":
        assert all(hp[b] >= pr.HASH_R_FILL + 1 for b in exp.overflow_buckets)
        held = set(((m.keys >> np.uint64(32 + 4))).astype(np.int64).tolist())
        assert held == set(range(256)) - (set(range(1, 71)) if args[0] else set())
    elif kind == "build_pair_capacity":
        assert cp == [0, chunk // 8 + args[0], 0]
    elif kind == "build_second_attempt":
        want = chunk * 9 // 2 + (28 if args[0] else 0)
        assert cp[1] == want and max(cp[0], cp[2]) == 0
        if args[0]:
            assert want > chunk * 9 // 2 and want <= (chunk + 7) * 9 // 2
            off = pr.read_bounds(rec)
            assert chunk in off and 2 * chunk - 1 in off and 2 * chunk not in off


def test_split_inputs():
    for n in (4096, 1024):
        rec, _, exp = pr.build_split_overflow(n)
        assert len(exp.overflow_buckets) == 1
        rec, _, exp = pr.build_split_big_read(n)
        assert pr.big_reads(rec) == 1 and pr.probe_wide_windows(rec, n) == 0
        assert max(pr.hash_pairs_per_bucket(rec, n).values()) <= 200
        assert max(pr.chunk_pairs(rec)) <= pr.CHUNK // 8
