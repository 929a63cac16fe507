"""tests/code_partition_reference.py without a GPU: the constants it restates
equal csrc/code_part.h, every case's records give the per-block, per-flush,
per-bucket histograms the case asked for (recomputed from the records alone,
for a geometry made by hand), each case sits on the limit it is named after,
and the plain model (pairs_reference.pair_graph) equals the oracle on the
cases' records, big-read filler included."""
import os
import re

import numpy as np
import pytest

import code_partition_reference as cp
import pairs_reference as pr
from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_geometry(name):
    n, chunks, knob = cp.case_geometry(name)
    lpb = min(cp.MAX_LISTS, -(-chunks // knob)) if knob else 1  # no knob: far more resident blocks than chunks
    return n, cp.geometry(n, chunks, lpb)


def test_constants_restate_the_header():
    hdr = open(os.path.join(REPO, "karma_amd", "csrc", "code_part.h")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, hdr).group(1))
    assert (val("kCodeFill"), val("kAppendCap"), val("kMaxListsPerBlock")) == (cp.CODE_FILL, cp.APPEND_CAP, cp.MAX_LISTS)
    assert (val("kNarrowBc"), val("kAppendMinBc"), val("kMaxBc")) == (cp.NARROW_BC, cp.APPEND_MIN_BC, cp.MAX_BC)
    assert (val("kCrPieces"), val("kCrSmax"), val("kCgShift")) == (cp.CR_PIECES, cp.CR_SMAX, cp.CG_SHIFT)
    assert 64 * val("kWin") == cp.ROUND_VECS and "kRoundVecs = 64 * kWin" in hdr
    assert cp.CODE_FILL % cp.CHUNK == 0 and cp.APPEND_CAP % cp.CHUNK == 0
    assert [cp.reduce_split(r) for r in (0, 1, 8, 9, 511, 512, 513)] == [1, 64, 64, 57, 2, 1, 1]
    assert [cp.staged_bound(cp.APPEND_CAP, nb) for nb in (293, 294, 300, 391, 512)] == [16384, 16400, 16488, 17760, 19456]
    assert [pr.geometry(n).Bc for n in cp.PATH2_N + cp.PATH3_N] == [57, 64, 65, 128, 129, 294, 391, 512]
    assert pr.geometry(262145).bwc == 12


@pytest.mark.parametrize("name", sorted(cp.CASES))
def test_case_meets_its_placement(name):
    n, geo = hand_geometry(name)
    rec = cp.case_records(name, geo)  # build() compares placement() with the histograms asked for
    assert len(rec) == geo.n_chunks * cp.CHUNK
    assert len(rec) < 300_000 or name.startswith("rows_51")  # 511 to 513 rows take as many chunks
    assert np.all(rec[1:, 0] >= rec[:-1, 0]) and int(rec[:, 1].max()) < n
    assert not pr.relabels(rec, n)
    got = cp.placement(rec, n, geo)
    assert len(got) == geo.n_pblk
    items = [int(sum(h.sum() for h in fl)) for fl in got]
    u = cp.usable(geo, n)
    cap = geo.flush
    kind = name.rsplit("_n", 1)[0]
    if kind.startswith("items_"):
        assert items == [cp.ITEMS[kind[6:]](cap), cap + 1234] and geo.lpb * cp.CHUNK >= max(items)
        assert [len(fl) for fl in got] == [-(-items[0] // cap), 2]
    elif kind == "one_bucket":
        assert [int(h.max()) for h in got[0]] == [cap, cap, 5] and cap - 1 < 1 << 16
    elif kind == "mod8_one":
        assert all(((h[:u] % 8) == 1).all() for h in got[0])
        assert (len(got[0]) == 2) == ((cap - u) % 8 == 0)
    elif kind == "residues":
        assert len(got[0]) == 3 and all(set(np.unique(h[:3 * u // 4] % 8)) == set(range(8)) for h in got[0])
        assert all((h[3 * u // 4:] == 0).all() for h in got[0])
    elif kind == "holes":
        assert [len(fl) for fl in got] == [1, 0, 2, 0] and items == [700, 0, cap + 3, 0]
    elif kind.startswith("lists_"):
        assert geo.lpb == cp.MAX_LISTS and items[0] == cp.MAX_LISTS * cp.CHUNK
        assert geo.n_pblk == (1 if kind == "lists_128" else 2)
    elif kind == "worst_case_regions":
        assert geo.path == 3 and cp.staged(got[0])[1] == cp.staged_bound(cap, u)
        assert (got[0][0][:u] % 8 == 7).sum() >= u - 1 and ((got[0][0] + got[0][1])[:u] % 8 == 1).all()
        # past the staging array's earlier size (cap + 8 * 512) wherever 294 buckets or more are usable
        assert (cp.staged(got[0])[1] > cap + 8 * cp.MAX_BC) == (u >= 294)
    elif kind.startswith("round_"):
        assert len(got) == 1 and len(got[0]) == 1 and -(-int(got[0][0][1]) // 8) == cp.ROUND_VECS + int(kind[6:])
    elif kind.startswith("rows_"):
        assert sum(len(fl) for fl in got) == geo.n_pblk == int(kind[5:]) and geo.lpb == 1
    else:
        raise AssertionError("a case without a pinned condition: " + name)


def test_usable_buckets():
    # the last bucket of 262,145, 524,289 and 1,200,129 contigs holds one contig, none below N - 3
    for n, u, short in zip(cp.PATH2_N + cp.PATH3_N, (57, 64, 64, 128, 128, 293, 391, 512), (0, 0, 1, 0, 1, 1, 0, 0)):
        g = cp.geometry(n, 1, 1)
        assert cp.usable(g, n) == u == g.Bc - short


def test_placement_refuses_a_flush_boundary_inside_a_list():
    n = 3648
    geo = cp.geometry(n, 6, 6)
    rng = np.random.default_rng(1)
    # chunk 0 holds 2,047 codes and one two-record read's worth of records: fine as the last chunk of a flush only
    ok = cp.build(geo, n, [[cp.random_hist(rng, geo.flush, geo, 57), cp.random_hist(rng, 2047, geo, 57)]])
    assert [int(h.sum()) for h in cp.placement(ok, n, geo)[0]] == [geo.flush, 2047]
    moved = np.concatenate([ok[4 * cp.CHUNK:5 * cp.CHUNK], ok[:4 * cp.CHUNK], ok[5 * cp.CHUNK:]])  # the short chunk first
    moved[:, 0] = np.cumsum(np.r_[True, moved[1:, 0] != moved[:-1, 0]]) - 1
    with pytest.raises(AssertionError, match="inside a list"):
        cp.placement(moved, n, geo)
    with pytest.raises(AssertionError):  # a flush that is not full and not the last
        cp.build(geo, n, [[cp.random_hist(rng, 100, geo, 57), cp.random_hist(rng, 100, geo, 57)]])


def test_shuffled_ids_call_for_the_relabel():
    rec = cp.shuffled_ids(524289, 60 * cp.CHUNK - 77)
    assert len(rec) == 60 * cp.CHUNK - 77 and pr.relabels(rec, 524289) and pr.big_reads(rec) == 0


@pytest.mark.parametrize("name", ["items_cap+1_n3648", "holes_n262145", "worst_case_regions_n1600000",
                                  "mod8_one_n4096", "round_+1_n524289"])
def test_model_equals_oracle_on_case_records(name):
    n, geo = hand_geometry(name)
    rec = cp.case_records(name, geo).astype(np.int64)
    m = pr.pair_graph(rec, n)
    o = oracle.graph_groups(pr.read_bounds(rec), rec[:, 1], None, None, n, dedup=True)
    assert np.array_equal(m.a, o["a"]) and np.array_equal(m.b, o["b"])
    assert np.array_equal(m.shared, o["shared"])
    assert np.array_equal(m.weight.view(np.uint64), o["weight"].view(np.uint64))
    assert np.array_equal(m.totals, o["totals"])
    # every compact read is one code: the totals' sum counts each record's contig once per read
    assert int(m.totals.sum()) == len(rec)
