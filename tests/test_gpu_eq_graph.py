"""The eq-class graph (csrc/eq.hip and the eq half of csrc/graph.hip) at every
constant that decides which code runs, one case on each side: kSmallM (32),
kSeg / kSegCap (1,024 / 2,048) and the run rule, the 32-lane probe of
run_start_g, the 512-position chunks of reduce_sorted_run, the 64-wide
look-back, the class search of eq_totals, the 4,096-item scan tiles and their
64-tile look-back, the 1,024-key blocks of the edge stage, the 256-edge blocks
and 4,096-entry chunks of eq_order, the speculative pair capacity, and the
limits of the compact input form.

Expected values come from oracle.graph_groups, which
tests/test_eq_reference_cpu.py pins to the plain model in tests/eq_reference.py
on these fixture families.  Every comparison is exact (weights as uint64 bit
patterns).  Each fixture asserts from the model's side (run_lengths, class
sizes, key positions, edge counts) that it sits where it claims to before the
device result is looked at.

Checked once against throw-away builds with one wrong comparison each (every
index kept in bounds); the tests that name the boundary and failed:
  pair_ij without "+ 1"                 test_class_size_alone[33..65], test_more_big_classes_than_compute_units_...
  LDS rank "q <= p"                     test_run_lengths_around_kSeg_and_kSegCap (the runs of <= 2,048)
  merge, right run "ka[m] < k"          test_run_lengths_around_kSeg_and_kSegCap[1023-1026], [1000-4097],
                                        test_group_of_equal_keys_straddles_a_512_chunk_edge[..-2100]
  every chunk's first position a head   test_group_of_equal_keys_straddles_a_512_chunk_edge[511-2, 510-3, 1023-2, 1022-3]
  run_start_g "segoff[p] <= target"     test_contig_counts_around_the_32_lane_probe (and every other case)
  eq_totals "off[mid] < j"              test_totals_empty_classes_single_members_and_negative_counts (and every other)
  eq_order "sf <= fi"                   test_insertion_order_of_a_run_around_the_block_and_the_chunk
  edge_flag without "c != 0"            test_pair_list_length_around_the_edge_block, test_every_sum_zero_gives_no_edges"""
import itertools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest

import eq_reference as R
from karma_amd import _lib, engine, synth
from karma_amd.read_graph import ReadGraph
from oracle import oracle

pytestmark = pytest.mark.gpu

FIELDS = ("a", "b", "shared", "first", "totals")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def size_scratch(ctx):
    """An empty call: it leaves the context's speculative pair capacity at 0, so
    the next call sizes its scratch from its own pair total (ceil(P / kSeg) runs)."""
    e = engine.graph_from_eq(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.int64),
                             np.zeros(0, np.uint8), 1, ctx=ctx)
    assert len(e.a) == 0


def same_edges(e, o):
    for k in FIELDS:
        assert np.array_equal(getattr(e, k), o[k]), k
    assert np.array_equal(bits(e.weight), bits(o["weight"]))


def same_ordered(got, o):
    order = np.lexsort((o["first"], o["a"]))
    a, b, w = got
    assert np.array_equal(a, o["a"][order]) and np.array_equal(b, o["b"][order])
    assert np.array_equal(bits(w), bits(o["weight"][order]))


def same_pair_list(case, ctx):
    """seg_reduce's own output, before the edge stage: distinct keys in order,
    their sums (zero sums included) and first emission indices."""
    off, mem, cnt, skip, n = case
    p = engine.Pairs.from_eq(ctx, off, mem, cnt, skip, n)
    try:
        got = p.get()
    finally:
        p.close()
    for g, w in zip(got, R.pair_list(off, mem, cnt, skip)):
        assert np.array_equal(g, w)
    return got


def check(case, ctx):
    """All fields through graph_from_eq on a sized scratch (the run lengths the
    fixtures assert) and on the capacity that call leaves (P + P / 8: empty tail
    runs), the pair list itself, the insertion order through
    graph_from_eq_ordered, and the compact form where the sizes and counts fit
    it.  Returns the oracle's result."""
    off, mem, cnt, skip, n = case
    o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
    assert not o["zero_div"]
    size_scratch(ctx)
    same_edges(engine.graph_from_eq(off, mem, cnt, skip, n, ctx=ctx), o)
    same_edges(engine.graph_from_eq(off, mem, cnt, skip, n, ctx=ctx), o)
    same_pair_list(case, ctx)
    same_ordered(engine.graph_from_eq_ordered(off, mem, cnt, skip, n, ctx=ctx), o)
    cq = engine.eq_compact(off, cnt, skip)
    if cq is not None:
        same_ordered(engine.graph_from_eq_compact_ordered(cq[0], mem, cq[1], n, ctx=ctx), o)
    return o


def packed(built):
    return R.pack(built[0]) + (built[1],)


# ---- class sizes: kSmallM = 32 --------------------------------------------------------

SIZES = [1, 2, 31, 32, 33, 34, 64, 65]


@pytest.mark.parametrize("dup", [False, True])
def test_class_sizes_on_both_sides_of_kSmallM_in_one_list(ctx, dup):
    case = packed(R.sized_classes(SIZES, dup))
    m = np.diff(case[0])
    assert all(s in m for s in SIZES) and int(np.sum(m > 32)) == 4 and int(np.sum(m == 32)) == 1
    o = check(case, ctx)
    assert bool(np.any(o["a"] == o["b"])) == dup  # the duplicates' self-pairs
    assert engine.eq_compact(case[0], case[2], case[3]) is not None


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("m", SIZES)
def test_class_size_alone(ctx, m, dup):
    case = packed(R.sized_classes([m], dup))
    assert int(np.diff(case[0]).max()) == max(m, 3)
    check(case, ctx)


def test_token_1_class_of_33_members_adds_totals_and_no_pairs(ctx):
    case = packed(R.sized_classes([33, 4], False, token1=(0,)))
    off, mem, cnt, skip, n = case
    c = int(np.flatnonzero(np.diff(off) == 33)[0])
    assert skip[c] == 1 and R.n_pairs(off, skip) == R.n_pairs(off, None) - 33 * 32 // 2
    o = check(case, ctx)
    members = mem[off[c]:off[c + 1]]
    without = oracle.graph_groups(off, mem, np.where(np.arange(len(cnt)) == c, 0, cnt), skip, n, dedup=False)
    assert np.array_equal(o["totals"][members] - without["totals"][members], np.full(33, cnt[c]))
    assert np.array_equal(o["shared"], without["shared"])


def test_more_big_classes_than_compute_units_first_is_the_combinations_index(ctx):
    case = packed(R.sized_classes([33] * 300, False, n=5000))
    off, mem, cnt, skip, n = case
    assert int(np.sum(np.diff(off) == 33)) == 300
    o = check(case, ctx)
    model = R.eq_model(off, mem, cnt, skip, n)
    assert len(model["a"]) > 150_000
    size_scratch(ctx)
    e = engine.graph_from_eq(off, mem, cnt, skip, n, ctx=ctx)
    assert np.array_equal(e.first, model["first"]) and np.array_equal(o["first"], model["first"])


# ---- run geometry: kSeg = 1,024, kSegCap = 2,048 ----------------------------------------

HUBS = [(0, 1023, [1023]), (0, 1024, [1024]), (1, 1023, [1024]), (1, 1024, [1025, 0]), (0, 1025, [1025, 0]),
        (1023, 1025, [2048, 0]), (1023, 1026, [2049, 0, 0]), (1, 2047, [2048, 0]),
        (1000, 4097, [5097, 0, 0, 0, 0])]


@pytest.mark.parametrize("prefix,hub,runs", HUBS)
def test_run_lengths_around_kSeg_and_kSegCap(ctx, prefix, hub, runs):
    """Runs of 1,023 to 2,048 entries rank in LDS, 2,049 (a power of two plus
    one) and 5,097 merge-sort in global scratch; groups of 2 to 5 equal keys and
    negative counts inside every run."""
    case = packed(R.hub_fixture(prefix, hub))
    off, mem, cnt, skip, n = case
    assert R.run_lengths(off, mem, skip, n) == runs
    keys = R.sorted_run_keys(off, mem, skip, 1)
    groups = {len(list(g)) for _, g in itertools.groupby(keys)}
    assert len(keys) == hub and groups >= {2, 3, 4, 5} and int(cnt.min()) < 0
    check(case, ctx)


def test_two_long_hubs_empty_runs_between_non_empty_ones(ctx):
    classes = R.star(0, R.grouped_partners(3000, 1), 1)
    classes += [([a, 100 + j], 2 + j % 3) for a in range(1, 21) for j in range(10)]
    classes += R.star(30, R.grouped_partners(2500, 31), 2)
    classes += [([a, 200 + j], 1 + j % 4) for a in range(40, 61) for j in range(10)]
    rng = np.random.default_rng(3)
    classes = [classes[i] for i in rng.permutation(len(classes))]
    n = 1 + max(x for c in classes for x in c[0])
    case = R.pack(classes + R.anchors(range(n))) + (n,)
    assert R.run_lengths(case[0], case[1], case[3], n) == [3000, 0, 80, 2620, 0, 210]
    check(case, ctx)


# ---- reduce_sorted_run: kRT = 512 positions per chunk -------------------------------------

@pytest.mark.parametrize("pos,group,L", [(511, 2, 1100), (510, 3, 1100), (512, 3, 1100),
                                         (1023, 2, 2100), (1022, 3, 2100), (1024, 3, 2100)])
def test_group_of_equal_keys_straddles_a_512_chunk_edge(ctx, pos, group, L):
    """L = 1,100: the LDS path; L = 2,100: the merge-sorted run, at position 1,024."""
    case = packed(R.straddle_fixture(pos, group, L))
    off, mem, cnt, skip, n = case
    assert R.run_lengths(off, mem, skip, n) == [L] + [0] * (-(-L // 1024) - 1)
    keys = R.sorted_run_keys(off, mem, skip, 0)
    edge = 512 if L <= R.K_SEG_CAP else 1024
    assert len(set(keys[pos:pos + group])) == 1 and pos <= edge <= pos + group - 1
    assert keys[pos - 1] != keys[pos] and keys[pos + group] != keys[pos] and len(keys) == L
    o = check(case, ctx)
    assert len(o["a"]) == L - group + 1
    keys = same_pair_list(case, ctx)[0]
    assert len(keys) == L - group + 1 and np.all(np.diff(keys.astype(np.int64)) > 0)  # one entry per key


# ---- run_start_g: 32-lane probe groups -----------------------------------------------------

@pytest.mark.parametrize("N", [1, 2, 32, 33, 34, 1024, 1025, 32_769])
def test_contig_counts_around_the_32_lane_probe(ctx, N):
    """No probe round for N <= 32, then 32-ary rounds; a few dozen active contigs
    spread over the id range, so run targets fall among tied segment offsets."""
    case = R.sparse_contigs(N)
    off, mem, cnt, skip, n = case
    active = np.unique(mem)
    assert R.n_pairs(off, skip) >= 3000 and len(active) <= 24 and int(active.max()) == N - 1
    runs = R.run_lengths(off, mem, skip, n)
    assert len(runs) == 3 and sum(runs) == 3000
    o = check(case, ctx)
    if N == 1:
        assert o["a"].tolist() == [0] and o["b"].tolist() == [0]  # the self-pair only


# ---- lookback_offset: 64 predecessors per round ------------------------------------------

@pytest.mark.parametrize("hub", [0, 3500])
def test_more_than_64_runs_through_the_look_back(ctx, hub):
    case = R.many_runs(80_000, 4000, hub=hub)
    off, mem, cnt, skip, n = case
    runs = R.run_lengths(off, mem, skip, n)
    filled = [i for i, x in enumerate(runs) if x]
    assert len(filled) >= 70 and R.n_pairs(off, skip) > 71_680
    if hub:  # runs without keys inside the 64-wide window of later runs
        empty = [i for i, x in enumerate(runs) if not x and 0 < i < filled[-1]]
        assert len(empty) >= 2 and max(runs) > R.K_SEG_CAP
        assert any(0 < f - empty[0] < 64 for f in filled)
    check(case, ctx)


# ---- eq_totals: the class of a member ----------------------------------------------------

def test_totals_empty_classes_single_members_and_negative_counts(ctx):
    case = packed(R.totals_fixture())
    off, mem, cnt, skip, n = case
    m = np.diff(off)
    assert m[0] == 0 and m[-1] == 0 and np.any((m[1:-1] == 0) & (m[2:] == 0)) and not skip.any()
    assert int(cnt.min()) == -2 ** 31 and np.any(cnt == 0)
    o = check(case, ctx)
    assert int(o["totals"].min()) < -2 ** 31 and not np.any(o["totals"][np.r_[o["a"], o["b"]]] == 0)
    # no skip array (NULL) and an all-zero one
    for sk in (np.zeros(0, np.uint8), np.zeros(len(cnt), np.uint8)):
        size_scratch(ctx)
        same_edges(engine.graph_from_eq(off, mem, cnt, sk, n, ctx=ctx), o)
        same_ordered(engine.graph_from_eq_ordered(off, mem, cnt, sk, n, ctx=ctx), o)
    o_null = oracle.graph_groups(off, mem, cnt, None, n, dedup=False)
    assert all(np.array_equal(o[k], o_null[k]) for k in FIELDS)


# ---- the scans: tiles of 4,096, look-back over 64 tiles -------------------------------------

@pytest.mark.parametrize("C", [4095, 4096, 4097, 270_000])
def test_class_and_contig_counts_around_the_scan_tile(ctx, C):
    """C classes over C contigs: the class-size scan and the pair-count scan run
    over C + 1 items, the segment scan over n + 1; 270,000 takes all three past
    64 tiles (262,144 items), in the wide form and in the compact one."""
    case = R.scan_tiles(C)
    assert len(case[0]) - 1 == C == case[4] and R.n_pairs(case[0], case[3]) == C
    assert engine.eq_compact(case[0], case[2], case[3]) is not None
    check(case, ctx)


# ---- the edge stage: kET = 1,024 keys per block -----------------------------------------------

@pytest.mark.parametrize("K", [1023, 1024, 1025, 2048, 2049])
def test_pair_list_length_around_the_edge_block(ctx, K):
    """Zero-sum keys at the last slot of block 0, the first slot of block 1, the
    last key of the list and in a run of 70 (more than a wave)."""
    zero = sorted({z for z in (1023, 1024) if z < K} | {K - 1} | set(range(100, 170)))
    case = packed(R.edge_fixture(K, zero_at=zero))
    off, mem, cnt, skip, n = case
    distinct = oracle.graph_groups(off, mem, np.ones_like(cnt), skip, n, dedup=False)
    assert len(distinct["a"]) == K  # the pair list: distinct keys, zero-sum ones included
    o = check(case, ctx)
    assert len(o["a"]) == K - len(zero)


def test_every_sum_zero_gives_no_edges(ctx):
    case = packed(R.edge_fixture(1500, zero_at=range(1500)))
    off, mem, cnt, skip, n = case
    o = check(case, ctx)
    assert len(o["a"]) == 0
    size_scratch(ctx)
    e = engine.graph_from_eq(off, mem, cnt, skip, n, ctx=ctx)
    a, b, w = engine.graph_from_eq_ordered(off, mem, cnt, skip, n, ctx=ctx)
    assert len(e.a) == len(e.weight) == len(a) == len(b) == len(w) == 0
    assert np.array_equal(e.totals, o["totals"])


@pytest.mark.parametrize("at", [3, 2048])
def test_kept_pair_over_a_zero_total_in_the_first_and_last_block(ctx, at, tmp_path):
    classes, n = R.edge_fixture(2049, zero_at=[7], zero_total_at=at)
    case = R.pack(classes) + (n,)
    off, mem, cnt, skip, _ = case
    o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
    ka, kb = R.edge_keys(2049)
    z = int(kb[at])
    assert o["zero_div"] and o["totals"][z] == 0 and np.count_nonzero(o["totals"] == 0) == 1
    # the pair list has 2,049 keys in three blocks; the one kept key of contig z is key `at`
    kept = np.flatnonzero((o["a"] == z) | (o["b"] == z))
    assert len(kept) == 1 and (int(o["a"][kept[0]]), int(o["b"][kept[0]])) == (int(ka[at]), z)
    assert at // 1024 == (0 if at == 3 else 2)
    for fn in (engine.graph_from_eq, engine.graph_from_eq_ordered):
        with pytest.raises(_lib.KarmaError) as ei:
            fn(off, mem, cnt, skip, n, ctx=ctx)
        assert ei.value.code == _lib.KARMA_ERR_ZERO_DIV, str(ei.value)
    names = [f"c{i}" for i in range(n)]
    p = tmp_path / "zero_total.txt"
    p.write_text(synth.eq_file_text(names, [(c[0], c[1]) for c in classes]))
    with pytest.raises(ZeroDivisionError):
        ReadGraph.from_equivalence_classes(str(p), OrderedDict((">" + x, "") for x in names))
    # both contexts work afterwards
    check(packed(R.edge_fixture(1025, zero_at=[1024])), ctx)
    check(packed(R.edge_fixture(1025, zero_at=[1024])), _lib.default_context())


# ---- eq_order: kOrdT = 256 edges per block, kOrdChunk = 4,096 per LDS chunk -----------------

@pytest.mark.parametrize("prefix", [0, 100])
@pytest.mark.parametrize("run", [255, 256, 257, 4095, 4096, 4097, 8193])
def test_insertion_order_of_a_run_around_the_block_and_the_chunk(ctx, run, prefix):
    classes, n, hub = R.order_fixture(run, prefix)
    case = R.pack(classes) + (n,)
    o = check(case, ctx)
    assert int(np.searchsorted(o["a"], hub)) == prefix and int(np.sum(o["a"] == hub)) == run
    first = o["first"][o["a"] == hub]
    assert np.any(np.diff(first.astype(np.int64)) < 0)  # emitted in shuffled order


def test_one_order_block_spans_more_than_100_short_runs(ctx):
    case = packed(R.short_runs())
    o = check(case, ctx)
    assert len(np.unique(o["a"][:256])) > 100 and len(o["a"]) > 512
    assert set(np.bincount(o["a"])[:300].tolist()) == {1, 2, 3}


# ---- graph_eq_run: the speculative pair capacity ------------------------------------------

def counted(ctx, fn):
    """fn()'s result and the seg_reduce launches it made."""
    ctx.timing(True, "seg_reduce")
    ctx.timing_reset()
    try:
        out = fn()
        n = ctx.timing_read().get("seg_reduce", (0.0, 0))[1]
    finally:
        ctx.timing(False)
    return out, n


def first_call_2048(c):
    """A fresh context's first call, 2,048 pairs: sized (one launch); leaves cap = 2,304."""
    off, mem, cnt, skip = R.two_member_classes(2048, 500, 1)
    e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 500, ctx=c))
    same_edges(e, oracle.graph_groups(off, mem, cnt, skip, 500, dedup=False))
    assert k == 1


@pytest.mark.parametrize("P2,launches", [(2303, 1), (2304, 1), (2305, 2)])
def test_speculative_capacity_edge(P2, launches):
    """cap = 2,048 + 2,048 / 8 = 2,304: a call of up to 2,304 pairs completes in
    one pass (below it with an empty tail run), one of 2,305 runs again, sized."""
    with _lib.Context(0) as c:
        first_call_2048(c)
        off, mem, cnt, skip = R.two_member_classes(P2, 700, 2)
        assert R.n_pairs(off, skip) == P2
        if P2 <= 2304:
            assert len(R.run_lengths(off, mem, skip, 700, cap=2304)) == 3
        o = oracle.graph_groups(off, mem, cnt, skip, 700, dedup=False)
        e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 700, ctx=c))
        assert k == launches
        same_edges(e, o)
        same_ordered(engine.graph_from_eq_ordered(off, mem, cnt, skip, 700, ctx=c), o)


def test_big_class_straddles_the_speculative_capacity():
    rng = np.random.default_rng(9)
    classes = [([int(x), int(y)], 3) for x, y in rng.integers(0, 600, (2000, 2))]
    classes.append((rng.choice(600, 33, replace=False).tolist(), 5))
    classes += [([int(x), int(y)], 2) for x, y in rng.integers(0, 600, (100, 2))]
    off, mem, cnt, skip = R.pack(classes)
    assert 2000 < 2304 < 2000 + 33 * 32 // 2 and R.n_pairs(off, skip) == 2628
    with _lib.Context(0) as c:
        first_call_2048(c)
        o = oracle.graph_groups(off, mem, cnt, skip, 600, dedup=False)
        e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 600, ctx=c))
        assert k == 2
        same_edges(e, o)


def test_three_pairs_after_150000_leave_all_runs_but_one_empty():
    with _lib.Context(0) as c:
        off, mem, cnt, skip = R.two_member_classes(150_000, 3000, 4)
        same_edges(engine.graph_from_eq(off, mem, cnt, skip, 3000, ctx=c),
                   oracle.graph_groups(off, mem, cnt, skip, 3000, dedup=False))
        off, mem, cnt, skip = R.pack([([7, 2], 4), ([2, 9], -1), ([9, 9], 3)])
        runs = R.run_lengths(off, mem, skip, 3000, cap=150_000 + 150_000 // 8)
        assert len(runs) == 165 and sorted(runs)[-2:] == [0, 3]
        o = oracle.graph_groups(off, mem, cnt, skip, 3000, dedup=False)
        e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 3000, ctx=c))
        assert k == 1
        same_edges(e, o)
        same_ordered(engine.graph_from_eq_ordered(off, mem, cnt, skip, 3000, ctx=c), o)


def test_calls_without_pairs_and_the_capacity_they_leave():
    """No pairs on a capacity of 0 (a fresh context, or after a call without
    pairs): no seg_reduce launch.  No pairs after a call with pairs is a call
    below the capacity: one pass over empty runs, and the next call is sized."""
    off, mem, cnt, skip = R.pack([([3], 5), ([], 2), ([1, 2], 7, 1)])  # members, totals, no pairs
    assert R.n_pairs(off, skip) == 0
    o = oracle.graph_groups(off, mem, cnt, skip, 500, dedup=False)
    with _lib.Context(0) as c:
        e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 500, ctx=c))
        assert k == 0
        same_edges(e, o)
        first_call_2048(c)
        e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 500, ctx=c))
        assert k == 1
        same_edges(e, o)
        e, k = counted(c, lambda: engine.graph_from_eq(off, mem, cnt, skip, 500, ctx=c))
        assert k == 0
        same_edges(e, o)
        first_call_2048(c)  # sized again: one launch


def test_compact_totals_on_a_speculative_capacity_wait_for_the_offset_scan():
    """On a speculative capacity the host never waits between the compact
    form's offset scan (main stream) and the totals kernel that searches those
    offsets (fork stream).  Small compact calls alternate with wide calls of
    other classes, so a totals kernel that ran early would search what an
    earlier call left in the buffer."""
    wide = R.sparse_contigs(2, P=2500, seed=3)
    rng = np.random.default_rng(12)
    classes = [(rng.choice(300, int(m), replace=False).tolist(), int(rng.integers(1, 9))) for m in
               rng.integers(1, 6, 900)]
    off, mem, cnt, skip = R.pack(classes)
    sz, c32 = engine.eq_compact(off, cnt, skip)
    o = oracle.graph_groups(off, mem, cnt, skip, 300, dedup=False)
    ow = oracle.graph_groups(*wide[:4], wide[4], dedup=False)
    with _lib.Context(0) as c:
        for _ in range(40):
            same_ordered(engine.graph_from_eq_ordered(*wide[:4], wide[4], ctx=c), ow)
            same_ordered(engine.graph_from_eq_compact_ordered(sz, mem, c32, 300, ctx=c), o)


# ---- bad offsets on the wide path ---------------------------------------------------------

def test_decreasing_middle_offset_is_an_argument_error(ctx):
    """off = [0, 4, 2, 6] over 6 members, n = 8, read kernel by kernel:
    scan_excl_pairs reads off[0..3] only; the sizes 4, -2, 4 give the pair counts
    6, (-2)(-3)/2 = 3, 6, so poff = [0, 6, 9, 15] and P = 15 (cap 15 when sized,
    or the earlier call's capacity; every pair index is checked against it).
    eq_rank_kernel: class 0 reads mem[0..3] and writes pairs 0..5; class 1 has
    e < s, sets bad |= 2 and writes rank = ~0 to pairs [6, min(9, cap)); class 2
    reads mem[2..5] (e = 6 <= n_mem = 6) and writes pairs 9..14, each only if
    below cap.  Nothing enters the big list.  eq_totals_kernel runs j = 0..5;
    its search keeps lo in [0, C) and reads off[1..2], cnt[lo] and mem[j], all
    inside, whatever the order of the offsets.  eq_place_kernel walks
    min(P, cap) pairs, skips the three sentinels, and puts the other 12 at
    segoff[a] + rank < 12 <= cap, a < N.  seg_reduce sees 12 placed pairs in one
    run.  The host then reports bad & 2."""
    off = np.array([0, 4, 2, 6], np.int64)
    mem = np.array([0, 1, 2, 3, 4, 5], np.uint32)
    cnt = np.array([2, 3, 4], np.int64)
    skip = np.zeros(3, np.uint8)
    for sized in (True, False):
        if sized:
            size_scratch(ctx)
        with pytest.raises(_lib.KarmaError) as ei:
            engine.graph_from_eq(off, mem, cnt, skip, 8, ctx=ctx)
        assert ei.value.code == _lib.KARMA_ERR_ARG and "disagree" in str(ei.value), str(ei.value)
        check(packed(R.sized_classes([2, 33], False)), ctx)  # the context is usable afterwards


# ---- the product boundary: which library entry ReadGraph takes -----------------------------

def product_case(tmp_path, monkeypatch, name, classes, n):
    names = [f"ctg{i}" for i in range(n)]
    p = tmp_path / f"{name}.txt"
    p.write_text(synth.eq_file_text(names, classes))
    fasta = OrderedDict((">" + x, "") for x in names)
    calls = {}
    monkeypatch.setattr(_lib, "CALL_TIMES", calls)
    g = ReadGraph.from_equivalence_classes(str(p), fasta)
    want = oracle.graph_from_eq_file(str(p), list(fasta))
    assert list(g.nodes()) == list(want.nodes())
    ge, we = list(g.edges(data="weight")), list(want.edges(data="weight"))
    assert [(a, b) for a, b, _ in ge] == [(a, b) for a, b, _ in we] and len(ge) > 0
    assert np.array_equal(bits([w for _, _, w in ge]), bits([w for _, _, w in we]))
    return {k for k in calls if k.startswith("karma_graph_eq")}


@pytest.mark.parametrize("members,entry", [(127, "karma_graph_eq_compact"), (128, "karma_graph_eq")])
def test_read_graph_takes_the_compact_entry_up_to_127_members(tmp_path, monkeypatch, members, entry):
    rng = np.random.default_rng(members)
    classes = [(rng.permutation(140)[:members].tolist(), 3), ([0, 5], 2), ([5, 139, 7], 11), ([9], 4)]
    assert product_case(tmp_path, monkeypatch, f"m{members}", classes, 140) == {entry}


@pytest.mark.parametrize("count,entry", [(2 ** 32 - 1, "karma_graph_eq_compact"), (2 ** 32, "karma_graph_eq")])
def test_read_graph_takes_the_compact_entry_up_to_u32_counts(tmp_path, monkeypatch, count, entry):
    classes = [([0, 1, 2], count), ([2, 3], 7), ([1, 0], count), ([4], 1), ([3, 3, 4], 2)]
    assert product_case(tmp_path, monkeypatch, f"c{count}", classes, 6) == {entry}


def test_read_graph_equals_the_reference_on_the_boundary_hand_cases(tmp_path):
    """tests/golden/eq_hand_boundary.json, the reference's own output
    (tests/golden/make_golden_eq_hand.py): nodes, edge order and weights."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eq_hand_boundary.json")) as f:
        cases = json.load(f)
    assert len(cases) == 4
    for name, case in cases.items():
        p = tmp_path / f"{name}.txt"
        p.write_text(case["text"])
        g = ReadGraph.from_equivalence_classes(str(p), OrderedDict((k, "") for k in case["fasta"]))
        assert isinstance(g, ReadGraph)
        assert [str(x) for x in g.nodes()] == case["out"]["nodes"], name
        assert [[str(a), str(b), float(d["weight"])] for a, b, d in g.edges(data=True)] == case["out"]["edges"], name
