"""CPU checks of tests/exchange_reference.py: the model against a brute-force
dict and against the CPU ops of the sharded build's rehearsal
(tests/test_distributed_cpu.py OracleOps), and every case builder against the
condition its name states.  No device calls."""
import numpy as np
import pytest

import exchange_reference as xr
from test_distributed_cpu import OracleOps


def brute(keys, counts):
    d = {}
    for k, c in zip(keys.tolist(), counts.tolist()):
        d[k] = d.get(k, 0) + c
    ks = sorted(d)
    return np.array(ks, np.uint64), np.array([d[k] for k in ks], np.int64)


def random_runs(seed, n, n_runs, n_contigs):
    rng = np.random.default_rng(seed)
    lens = np.diff(np.r_[0, np.sort(rng.integers(0, n + 1, n_runs - 1)), n]).tolist()
    a = rng.integers(0, n_contigs, n)
    b = np.minimum(a + rng.integers(0, 4, n), n_contigs - 1)
    keys = xr.key(a, b)
    off = np.r_[0, np.cumsum(lens)]
    for r in range(n_runs):
        keys[off[r]:off[r + 1]] = np.sort(keys[off[r]:off[r + 1]])
    return keys, rng.integers(-5, 50, n).astype(np.int64), lens


@pytest.mark.parametrize("seed,n,n_runs,n_contigs", [(1, 0, 3, 5), (2, 1, 1, 5), (3, 500, 4, 40), (4, 3000, 70, 90)])
def test_model_equals_brute_force(seed, n, n_runs, n_contigs):
    keys, counts, lens = random_runs(seed, n, n_runs, n_contigs)
    u, c = xr.merge(keys, counts, lens)
    bu, bc = brute(keys, counts)
    assert np.array_equal(u, bu) and np.array_equal(c, bc)
    # split: the first key whose a reaches the bound, by a linear scan
    a = (u >> np.uint64(32)).astype(np.int64)
    bounds = [0, 1, n_contigs // 2, n_contigs // 2, n_contigs - 1, n_contigs]
    assert xr.split(u, bounds).tolist() == [int((a < x).sum()) for x in bounds]
    # totals and edges, one key at a time
    tot = [0] * n_contigs
    for k, s in zip(bu.tolist(), bc.tolist()):
        if k >> 32 == k & 0xFFFFFFFF:
            tot[k >> 32] = s
    assert xr.totals(keys, counts, n_contigs).tolist() == tot
    for mode, given in ((xr.READS, None), (xr.EQ, [7 * (i % 3) for i in range(n_contigs)])):
        t = tot if given is None else given
        rows, zero = [], False
        for k, s in zip(bu.tolist(), bc.tolist()):
            x, y = k >> 32, k & 0xFFFFFFFF
            if s == 0 or (x == y and mode == xr.READS):
                continue
            if t[x] == 0 or t[y] == 0:
                zero = True
                rows.append((x, y, s, 0.0))
            else:
                rows.append((x, y, s, (float(s) / float(t[x]) + float(s) / float(t[y])) / 2))
        m = xr.edges(keys, counts, n_contigs, mode, given)
        assert m.zero_div == zero and m.totals.tolist() == list(t)
        assert list(zip(m.a.tolist(), m.b.tolist(), m.shared.tolist(), m.weight.tolist())) == rows


def test_model_equals_the_rehearsal_ops():
    ops = OracleOps()
    keys, counts, lens = random_runs(9, 4000, 5, 60)
    counts = np.abs(counts) + 1
    # every contig's diagonal, so that no total is 0 (the ops divide by it)
    d = np.arange(60)
    keys = np.r_[keys, xr.key(d, d)]
    counts = np.r_[counts, 100 + d]
    lens = lens + [60]
    u, c = xr.merge(keys, counts, lens)
    o = ops.merge(keys.view(np.int64).copy(), counts.copy(), lens)
    assert np.array_equal(o["keys"], u) and np.array_equal(o["counts"], c)
    assert np.array_equal(ops.totals(o, 60), xr.totals(u, c, 60))
    for given in (None, 1 + np.arange(60) * 3):
        e, m = ops.edges(o, 60, given), xr.edges(keys, counts, 60, xr.READS, given)
        assert not m.zero_div and len(m.a) > 100
        assert np.array_equal(e["a"], m.a) and np.array_equal(e["b"], m.b) and np.array_equal(e["shared"], m.shared)
        assert np.array_equal(e["weight"].view(np.uint64), m.weight.view(np.uint64))
        assert np.array_equal(e["totals"], m.totals)
    bounds = [0, 7, 7, 30, 60]
    assert np.array_equal(ops.pairs_kv(o, bounds)[2], xr.split(u, bounds))


@pytest.mark.parametrize("name", sorted(xr.CASES) + sorted(xr.UNSORTED))
def test_case_builder_conditions(name):
    c = xr.case(name)  # the builder asserts what its name says
    assert c.sorted == (name in xr.CASES)
    a, b = xr.ab(c.keys)
    assert not len(a) or (np.all(a <= b) and b.max() < c.N)
    assert len(c.keys) <= 110_000
    if c.sorted:
        sk, sc = xr.stable_merge(c.keys, c.counts, c.runs)
        u, s = xr.case_model(name)
        assert np.array_equal(np.unique(sk), u) and int(sc.sum()) == int(s.sum())


def test_constants_are_the_kernels():
    assert (xr.TILE, xr.LDS, xr.MAX_RUNS, xr.MG) == (1024, 6144, 64, 16)
    assert xr.BOUND_L == (1, 15, 16, 17, 31, 33, 255, 256, 257, 272, 273, 4097)


def test_tile_edge_cases():
    assert xr.case("tile_lengths").runs == [1, 1023, 1024, 1025, 2048, 2049]
    runs = xr.case("empty_first_middle_last").runs
    assert runs[0] == runs[2] == runs[4] == 0 and runs[1] and runs[3] > xr.TILE
    assert xr.case("all_empty").runs == [0] * 4 and xr.windows(xr.case("all_empty").keys, [0] * 4) == []
    assert len(xr.case("one_run").runs) == 1
    for W in (2, 3, 63, 64):
        c = xr.case(f"ties_{W}")
        assert len(c.runs) == W and len(xr.case_model(f"ties_{W}")[0]) == c.runs[0] == 1025
    c = xr.case("all_identical")
    assert c.runs == [1025] * 64 and len(np.unique(c.keys)) == 1
    c = xr.case("repeat_in_run")
    off = np.r_[0, np.cumsum(c.runs)]
    run1 = c.keys[off[1]:off[2]]
    assert run1[1023] == run1[1024] and (np.diff(run1) == 0).sum() > 400
    assert np.isin(run1, c.keys[:off[1]]).all()


def test_window_cases_hit_the_stage_limit():
    for name, lens, staged, inplace in [
            ("window_6143", [6143], [1], []), ("window_6144", [6144], [1], []), ("window_6145", [6145], [], [1]),
            ("window_3072_3072", [3072, 3072], [1, 2], []), ("window_3072_3073", [3072, 3073], [1], [2]),
            ("window_spill_then_small", [6145, 10], [2], [1]),
            ("window_spill_between", [4000, 3000, 2144], [1, 3], [2])]:
        bl = xr.window_block0(name)
        assert (bl.run, bl.tile, bl.lens[1:], bl.staged, bl.inplace) == (0, 0, lens, staged, inplace), name
        assert bl.used == sum(bl.lens[s] for s in staged) <= 6144
    assert xr.window_block0("window_6144").used == xr.window_block0("window_spill_between").used == 6144


def test_window_model_on_a_hand_case():
    # run 0: 10 20 30; run 1: 5 20 20 30 40; run 2: 20 30 30
    keys = np.array([10, 20, 30, 5, 20, 20, 30, 40, 20, 30, 30], np.uint64)
    runs = [3, 5, 3]
    b0, b1, b2 = xr.windows(keys, runs)
    # run 0's tile 10..30 against later runs (<): run 1 has 1 key < 10 and 3 keys < 30; run 2: 0 and 1
    assert b0.lens == [0, 2, 1]
    # run 1's tile 5..40: run 0 before it (<=): 0 and 3; run 2 after it (<): 0 and 3
    assert b1.lens == [3, 0, 3]
    # run 2's tile 20..30: runs before it (<=): run 0: 2 and 3; run 1: 3 and 4
    assert b2.lens == [1, 1, 0]
    assert xr.rank_counts(keys, runs, 0, 1).tolist() == [1, 1, 3]
    assert xr.rank_counts(keys, runs, 2, 0).tolist() == [2, 3, 3]


def test_launch_model():
    assert xr.merge_launches([5, 0, 7]) == {"merge_bounds": 1, "merge_rank": 1, "merge_split": 0,
                                            "merge_groups": 1, "merge_sum": 1}
    assert xr.merge_launches([5, 0, 7], kc=True, lazy=True)["merge_groups"] == 0
    assert not any(xr.merge_launches([0, 0], lazy=True).values()) and not any(xr.merge_launches([0, 0]).values())
    # one pair per non-lone, non-empty group per level; the wire format is split once
    for name, levels, pairs in (("runs_65", 2, 1 + 1), ("runs_129", 2, 1 + 1), ("runs_4097", 3, 63 + 1 + 1)):
        c = xr.case(name)
        assert xr.merge_levels(len(c.runs)) == levels
        want = {"merge_bounds": pairs, "merge_rank": pairs, "merge_split": 0, "merge_groups": 1, "merge_sum": 1}
        assert xr.merge_launches(c.runs) == xr.merge_launches(c.runs, lazy=True) == want, name
        assert xr.merge_launches(c.runs, kc=True) == dict(want, merge_split=1)
    c = xr.case("runs_4097")
    assert sum(c.runs[128:192]) == 0 and 0 in c.runs[:64] and any(c.runs[:64])
    assert sum(xr.case("runs_129").runs[64:128]) == 0


def test_edge_case_shapes():
    for name, n_past in (("totals_last_plus_1", 1), ("totals_last_plus_2", 2), ("totals_last_plus_5000", 5000)):
        for suffix, zero in (("", False), ("_zero_div", True)):
            c, m = xr.case(name + suffix), xr.case_edges(name + suffix)
            a = np.unique(xr.ab(c.keys)[0])
            assert c.N == a[-1] + n_past and a[0] == 7 and m.zero_div == zero
            assert len(xr.case_model(name + suffix)[0]) < len(c.keys)  # unsummed groups
    for name in ("slice", "slice_zero_div"):
        c = xr.case(name)
        a = xr.ab(c.keys)[0]
        assert c.N == 100_000 and a.min() >= 40_000 and a.max() < 41_000
    assert xr.case_edges("slice_zero_div").b.max() >= 41_000 > xr.case_edges("slice").b.max()
    for name, n in (("edges_n_1023", 1023), ("edges_n_1024", 1024), ("edges_n_1025", 1025)):
        assert len(xr.case(name).keys) == len(xr.case_model(name)[0]) == n
    k, _ = xr.stable_merge(*[getattr(xr.case("edges_group_across_blocks"), f) for f in ("keys", "counts", "runs")])
    assert k[1021] != k[1022] == k[1023] == k[1024] == k[1025] != k[1026]
    m = xr.case_edges("edges_diagonals_only")
    assert len(m.a) == 0 and np.count_nonzero(m.totals) > 1024
    m = xr.case_edges("weights")
    assert xr.case("weights").recip_differ >= 100 and m.shared.max() > 1 << 53 and m.totals.max() > 1 << 53


def test_dealing_a_list_to_runs_keeps_it():
    rng = np.random.default_rng(3)
    u = xr.G(np.arange(501))
    cnt = rng.integers(0, 3, 501).astype(np.int64) * 1000
    k, c = xr.with_dups(u, cnt, rng)
    assert len(k) > len(u) and np.array_equal(xr.merge(k, c)[1], cnt)
    assert np.all(c[np.isin(k, u[cnt == 0]) & (np.r_[k[1:] == k[:-1], False] | np.r_[False, k[1:] == k[:-1]])] != 0)
    keys, counts, lens = xr.to_runs(k, c, 3, rng)
    assert xr.sorted_runs(keys, lens) and sum(lens) == len(k)
    assert np.array_equal(xr.stable_merge(keys, counts, lens)[0], k)
