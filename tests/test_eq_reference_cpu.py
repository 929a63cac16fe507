"""Pins oracle.graph_groups(..., dedup=False) -- the expected values of
tests/test_gpu_eq_graph.py -- to tests/eq_reference.py's eq_model, the plain
restatement of read_graph.py:86-131: every field, the weights as bit patterns
and the zero-division flag, on seeded small inputs and on every fixture family
of the GPU file at its smallest size; and run_lengths on hand-computed cases.
The oracle is also held to the reference's own output on four more hand cases
(tests/golden/eq_hand_boundary.json).  No GPU calls."""
import json
import os

import numpy as np
import pytest

import eq_reference as R
from oracle import oracle

N_INPUTS = 240


def same(off, mem, cnt, skip, n, zero_div=False):
    m = R.eq_model(off, mem, cnt, skip, n)
    o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
    for k in ("a", "b", "shared", "first", "totals"):
        assert np.array_equal(m[k], o[k]) and m[k].dtype == o[k].dtype, k
    assert np.array_equal(m["weight"].view(np.uint64), o["weight"].view(np.uint64))
    assert m["zero_div"] == o["zero_div"] == zero_div
    # the vectorised pair list (what Pairs.get() is compared with) against the dict's
    for got, want in zip(R.pair_list(off, mem, cnt, skip), m["pairs"]):
        assert np.array_equal(got, want) and got.dtype == want.dtype
    return m


def random_case(seed):
    """Class sizes 0 to 40, duplicate members, skip flags on classes of several
    members, negative and zero counts, sparse contig ids."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    ids = np.unique(rng.integers(0, n, int(rng.integers(1, 30))))  # the contigs in use
    classes = []
    for _ in range(int(rng.integers(0, 25))):
        m = int(rng.choice([0, 1, 2, 2, 3, 4, int(rng.integers(0, 41))]))
        mem = ids[rng.integers(0, len(ids), m)].tolist()  # with replacement: duplicates
        cnt = int(rng.choice([0, 1, -1, 6, -6, int(rng.integers(-50, 50)), 2 ** 31, -2 ** 31]))
        classes.append((mem, cnt, int(rng.random() < 0.2)))
    return R.pack(classes) + (n,)


@pytest.mark.parametrize("block", range(4))
def test_oracle_equals_model_seeded(block):
    seen = dict(zero_div=0, skipped_big=0, dup=0, dropped=0)
    for seed in range(7000 + block * N_INPUTS // 4, 7000 + (block + 1) * N_INPUTS // 4):
        off, mem, cnt, skip, n = random_case(seed)
        m = R.eq_model(off, mem, cnt, skip, n)
        same(off, mem, cnt, skip, n, zero_div=m["zero_div"])
        seen["zero_div"] += m["zero_div"]
        seen["skipped_big"] += int(np.any((np.diff(off) > 2) & (skip != 0)))
        seen["dup"] += int(np.any(m["a"] == m["b"]))
        # distinct pairs (every count 1) that the real counts sum to 0
        seen["dropped"] += int(len(m["a"]) < len(R.eq_model(off, mem, np.ones_like(cnt), skip, n)["a"]))
    # the draw reaches what it claims to (each block of 60 inputs)
    assert all(seen.values()), seen


def test_no_skip_array_equals_zero_flags():
    off, mem, cnt, skip, n = random_case(7003)
    a = R.eq_model(off, mem, cnt, None, n)
    b = R.eq_model(off, mem, cnt, np.zeros(len(cnt), np.uint8), n)
    o = oracle.graph_groups(off, mem, cnt, None, n, dedup=False)
    for k in ("a", "b", "shared", "first", "totals"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], o[k])


def packed(built):
    classes, n = built[0], built[1]
    return R.pack(classes) + (n,)


# every fixture family of tests/test_gpu_eq_graph.py at its smallest size
FAMILIES = {
    "sizes_all": lambda: packed(R.sized_classes([1, 2, 31, 32, 33, 34, 64, 65], False)),
    "sizes_all_dup": lambda: packed(R.sized_classes([1, 2, 31, 32, 33, 34, 64, 65], True)),
    "size_33_alone_dup": lambda: packed(R.sized_classes([33], True)),
    "token1_33": lambda: packed(R.sized_classes([33, 4], False, token1=(0,))),
    "big_300x33": lambda: packed(R.sized_classes([33] * 300, False, n=5000)),
    "hub_0_1023": lambda: packed(R.hub_fixture(0, 1023)),
    "hub_1023_1026": lambda: packed(R.hub_fixture(1023, 1026)),
    "hub_1000_4097": lambda: packed(R.hub_fixture(1000, 4097)),
    "straddle_511_2": lambda: packed(R.straddle_fixture(511, 2, 1100)),
    "straddle_1022_3_merge": lambda: packed(R.straddle_fixture(1022, 3, 2100)),
    "sparse_N1": lambda: R.sparse_contigs(1),
    "sparse_N33": lambda: R.sparse_contigs(33),
    "sparse_N1025": lambda: R.sparse_contigs(1025),
    "many_runs_small": lambda: R.many_runs(6000, 300, hub=2100),
    "totals": lambda: packed(R.totals_fixture()),
    "scan_4097": lambda: R.scan_tiles(4097),
    "edges_1023": lambda: packed(R.edge_fixture(1023, zero_at=[5, 1022])),
    "edges_all_zero": lambda: packed(R.edge_fixture(1023, zero_at=range(1023))),
    "order_255": lambda: packed(R.order_fixture(255, 100)),
    "short_runs": lambda: packed(R.short_runs()),
}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_oracle_equals_model_on_fixture(name):
    off, mem, cnt, skip, n = FAMILIES[name]()
    m = same(off, mem, cnt, skip, n)
    if name == "edges_all_zero":
        assert len(m["a"]) == 0
    if name == "big_300x33":
        assert len(m["a"]) > 150_000


def test_zero_total_fixture_sets_the_flag():
    for at in (3, 2048):
        off, mem, cnt, skip, n = packed(R.edge_fixture(2049, zero_at=[7], zero_total_at=at))
        m = same(off, mem, cnt, skip, n, zero_div=True)
        a, b = R.edge_keys(2049)
        assert m["totals"][b[at]] == 0 and np.count_nonzero(m["totals"] == 0) == 1


def test_run_lengths_by_hand():
    # no pairs: one empty run; 3 + 1 pairs; a capacity beyond the pairs adds empty tail runs
    assert R.run_lengths([0], [], None, 4) == [0]
    off, mem, cnt, skip = R.pack([([0, 1, 2], 1), ([2, 3], 1)])
    assert R.run_lengths(off, mem, skip, 4) == [4]
    assert R.run_lengths(off, mem, skip, 4, cap=2049) == [4, 0, 0]
    # segments of 600 pairs on contigs 0, 1, 2: lo(1) is the first segment start >= 1024 (1200), lo(2) = P
    off, mem, cnt, skip = R.pack([([a, 3], 1) for a in (0, 1, 2) for _ in range(600)])
    assert R.run_lengths(off, mem, skip, 4) == [1200, 600]
    # a segment start exactly on 1024 opens run 1 there
    off, mem, cnt, skip = R.pack([([0, 3], 1)] * 1024 + [([1, 3], 1)] * 10)
    assert R.run_lengths(off, mem, skip, 4) == [1024, 10]
    # ... and one entry earlier it does not: run 0 takes both segments
    off, mem, cnt, skip = R.pack([([0, 3], 1)] * 1023 + [([1, 3], 1)] * 10)
    assert R.run_lengths(off, mem, skip, 4) == [1033, 0]
    # skipped classes and single members emit nothing
    off, mem, cnt, skip = R.pack([([0, 1, 2], 1, 1), ([3], 5), ([1, 2], 1)])
    assert R.run_lengths(off, mem, skip, 4) == [1]
    # the hub fixtures (one segment of `prefix` pairs before the hub)
    for prefix, hub, want in ((0, 1025, [1025, 0]), (1023, 1025, [2048, 0]), (1023, 1026, [2049, 0, 0]),
                              (1, 2047, [2048, 0]), (1000, 4097, [5097, 0, 0, 0, 0]), (0, 1023, [1023]),
                              (0, 1024, [1024]), (1, 1023, [1024]), (1, 1024, [1025, 0])):
        off, mem, cnt, skip, n = packed(R.hub_fixture(prefix, hub))
        assert R.run_lengths(off, mem, skip, n) == want, (prefix, hub)


def boundary_hand_cases():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eq_hand_boundary.json")) as f:
        return json.load(f)


def test_oracle_equals_the_reference_on_the_boundary_hand_cases(tmp_path):
    """The reference's own graphs (tests/golden/make_golden_eq_hand.py): a class of
    34 with a duplicate member, a pair revived after its sum returned to 0 (placed
    by its first emission), a pair ending at 0 between kept ones, a size-token-"1"
    class of three members.  Nodes, networkx edge order and weights."""
    cases = boundary_hand_cases()
    assert len(cases) == 4
    for name, case in cases.items():
        p = tmp_path / f"{name}.txt"
        p.write_text(case["text"])
        d = oracle.graph_dump(oracle.graph_from_eq_file(str(p), case["fasta"]))
        assert d["edges"] == case["out"]["edges"], name
        assert d["nodes"] == case["out"]["nodes"], name  # every FASTA name is an eq name: no set order involved
    assert len(cases["class_of_34_one_duplicate"]["out"]["edges"]) == 530
    assert [e[:2] for e in cases["zero_sum_pair_revived"]["out"]["edges"][:3]] == [["a", "c"], ["a", "b"], ["a", "d"]]
    assert [e[:2] for e in cases["zero_sum_pair_between_kept"]["out"]["edges"]] == [["a", "b"], ["a", "d"], ["c", "d"]]
