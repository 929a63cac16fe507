"""CPU checks of tests/step_tail_reference.py: the model against the oracle
(oracle.graph_groups) and a brute-force dict (pairs_reference.pair_graph) on
every family of batches, the restated device rules against direct scans, and
every builder against the condition its name states.  No device calls."""
import numpy as np
import pytest

import exchange_reference as xr
import pairs_reference as pr
import step_tail_reference as st
from oracle import oracle


def oracle_graph(rec, n):
    rs = np.asarray(rec, np.int64).reshape(-1, 2)
    return oracle.graph_groups(pr.read_bounds(rs), rs[:, 1], None, None, n, dedup=True)


def check_model(recs, batches, N, brute=True):
    """The union of the ranks' records: read ids made distinct across ranks."""
    parts, base = [], 0
    for r in recs:
        r = np.asarray(r, np.int64).reshape(-1, 2).copy()
        r[:, 0] += base
        base = int(r[-1, 0]) + 1 if len(r) else base
        parts.append(r)
    rec = np.concatenate(parts)
    m = st.graph(batches, N)
    refs = [oracle_graph(rec, N)]
    if brute:
        b = pr.pair_graph(rec, N)
        refs.append(dict(a=b.a, b=b.b, shared=b.shared, weight=b.weight, totals=b.totals))
        lists = [st.pair_list(x) for x in batches]
        u, c = xr.merge(np.concatenate([k for k, _ in lists]), np.concatenate([c for _, c in lists]))
        assert np.array_equal(u, b.keys) and np.array_equal(c, b.counts)
    for o in refs:
        assert np.array_equal(m.a, o["a"]) and np.array_equal(m.b, o["b"])
        assert np.array_equal(m.shared, o["shared"])
        assert np.array_equal(m.weight.view(np.uint64), np.asarray(o["weight"]).view(np.uint64))
        assert np.array_equal(m.totals, o["totals"])
    assert not m.zero_div


def check_deferred_prediction(rec, N):
    """The vectorised verdict against pairs_reference's read-by-read ones."""
    assert st.stays_deferred(rec, N)
    assert pr.big_reads(rec) == 0 and not pr.relabels(rec, N)
    assert not pr.hash_pairs_per_bucket(rec, N) and not any(True for _ in pr.general_reads(rec))


@pytest.mark.parametrize("name", sorted(st.EMU_CASES))
def test_emulated_case_model_and_placement(name):
    c = st.emu_case(name)  # the builder asserts its own placement
    check_model([c.rec], [c.batch], c.N)
    check_deferred_prediction(c.rec, c.N)
    for i, d in enumerate(c.dirt):
        rec = st.records(d, i)
        assert st.stays_deferred(rec, c.N)
        m = st.graph([d], c.N)
        assert m.totals.all() and len(rec) > 0           # every contig a nonzero total
        k = st.pair_list(d)[0]
        tiles = np.bincount(np.searchsorted(k, xr.key(m.a, m.b)) // st.ET, minlength=-(-len(k) // st.ET))
        assert tiles.all() and len(k) == st.dirt_keys(c.N) > c.U   # every edge tile counts edges; a longer list
    # the run offsets, by a linear scan
    k = st.pair_list(c.batch)[0]
    a = xr.ab(k)[0]
    scan = [int((a < bd).sum()) for bd in c.bounds]
    if len(c.bounds) > 2:
        assert st.run_offsets(k, c.bounds, c.N).tolist() == scan


def test_stays_deferred_rejects_what_it_should():
    ok = st.records(st.chain(np.arange(50)))
    assert st.stays_deferred(ok, 50)
    wide = np.array([[0, 3], [0, 7]], np.uint32)          # span 4: a general read
    assert not st.stays_deferred(wide, 50) and any(True for _ in pr.general_reads(wide))
    big = np.array([[0, c % 3] for c in range(9)], np.uint32)
    assert not st.stays_deferred(big, 50) and pr.big_reads(big) == 1
    assert not st.stays_deferred(ok, 49)                  # a contig id past the range


def brute_windows(keys, runs):
    """(run, tile) -> per run the keys counted before the tile's last key less
    those before its first, by linear scans."""
    off = np.r_[0, np.cumsum(runs)]
    out = {}
    for r in range(len(runs)):
        for t in range(-(-runs[r] // st.MT)):
            t0 = off[r] + t * st.MT
            t1 = min(off[r + 1], t0 + st.MT)
            lens = []
            for s in range(len(runs)):
                run = keys[off[s]:off[s + 1]]
                if s == r:
                    lens.append(0)
                elif s < r:
                    lens.append(max(0, int((run <= keys[t1 - 1]).sum()) - int((run <= keys[t0]).sum())))
                else:
                    lens.append(max(0, int((run < keys[t1 - 1]).sum()) - int((run < keys[t0]).sum())))
            out[(r, t)] = lens
    return out


@pytest.mark.parametrize("name", sorted(st.RANK_CASES))
def test_rank_case_model_and_placement(name):
    c = st.rank_case_named(name)  # the builder asserts its own placement
    check_model(c.recs, c.batches, c.N)
    for rec in c.recs:
        check_deferred_prediction(rec, c.N)
    # the owners' runs cover every rank's list, and the window arithmetic holds by scan
    total = 0
    for r in range(c.W):
        k, cnt, runs = st.owner_runs(c.batches, c.bounds, c.N, r)
        total += len(k)
        a = xr.ab(k)[0]
        assert not len(k) or (a.min() >= c.bounds[r] and a.max() < c.bounds[r + 1])
        if r == 0 or c.W <= 3:
            bw = brute_windows(k, runs)
            for bl in st.windows(k, runs):
                assert bl.lens == bw[(bl.run, bl.tile)], (name, r, bl.run, bl.tile)
                assert bl.used == sum(bl.lens[s] for s in bl.staged) <= st.MLDS
                assert bl.fast == (not bl.inplace and len(runs) <= st.MFAST)
    assert total == sum(len(st.pair_list(b)[0]) for b in c.batches)
    # the slot the sizing step leaves, from the definition
    mx = 0
    for b in c.sizing:
        a = xr.ab(st.pair_list(b)[0])[0]
        mx = max(mx, max(int(((a >= lo) & (a < hi)).sum()) for lo, hi in zip(c.bounds, c.bounds[1:])))
    assert c.kc == mx + mx // 4 + 1024
    assert (c.mx > c.kc) == c.rerun and c.rerun == (name == "slot_kc_plus_1")


def test_window_cases_cover_the_sizes_asked_for():
    seen = set()
    for name in st.RANK_CASES:
        if name.startswith("window_"):
            seen |= set(st.owner_tiles(st.rank_case_named(name))[0][0].lens)
    want = {0, 1, 2, 3, 4, st.MLDS - 1, st.MLDS, st.MLDS + 1} | {2 ** j - 1 for j in range(3, 11)} | \
        {2 ** j for j in range(3, 11)}
    assert want <= seen
    bl = st.owner_tiles(st.rank_case_named("window_1_and_5000"))[0][0]
    assert bl.lens[1:] == [1, 5000] and bl.fast         # the search's step count comes from the larger window
    bl = st.owner_tiles(st.rank_case_named("window_spill_then_small"))[0][0]
    assert bl.inplace == [1] and bl.staged == [2] and bl.used == 10


def test_large_cases_model_and_placement():
    """The cases sized by the device's grid caps, at a 256-CU device's (the GPU
    test builds them from the export): against the oracle alone (vectorised)."""
    c = st.build_second_round()
    check_model([c.rec], [c.batch], c.N, brute=False)
    assert st.stays_deferred(c.rec, c.N)
    assert -(-c.U // st.ET) == st.EDGE_BLOCKS + 2
    # the model again through the other vectorised path on a dirtying batch
    d = c.dirt[1]
    check_model([st.records(d, 1)], [d], c.N, brute=False)
