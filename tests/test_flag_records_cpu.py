"""engine.flag_records ((read, contig) records -> KARMA_REC_FLAGGED words)
against a plain Python loop, and the inputs it must refuse: the flagged words
no longer carry read ids, so records that are not grouped by read (ids A, B, A)
would silently become three reads -- flag_records is the last place that can
see it (the pairs format reports KARMA_ERR_UNSORTED for the same records)."""
import numpy as np
import pytest

from karma_amd import engine


def plain(records):
    """contig | (first record of its read) << 31, one record at a time."""
    out, prev = [], None
    for read, contig in records:
        read, contig = int(read), int(contig)
        assert 0 <= contig < 1 << 31
        out.append(contig | ((1 << 31) if prev is None or read != prev else 0))
        prev = read
    return out


def check(records):
    w = engine.flag_records(records)
    assert w.dtype == np.uint32 and w.ndim == 1
    assert w.tolist() == plain(np.asarray(records, np.int64).reshape(-1, 2).tolist())
    return w


def test_empty_one_record_one_read():
    assert check(np.zeros((0, 2), np.uint32)).tolist() == []
    assert check([]).tolist() == []
    assert check([(7, 5)]).tolist() == [5 | 1 << 31]
    assert check([(7, 0)]).tolist() == [1 << 31]
    assert check([(3, 4), (3, 9), (3, 4), (3, 0)]).tolist() == [4 | 1 << 31, 9, 4, 0]


def test_one_record_reads_and_runs_of_equal_ids():
    rng = np.random.default_rng(0)
    n = 1000
    ones = np.stack([np.arange(n), rng.integers(0, 500, n)], 1).astype(np.uint32)
    w = check(ones)
    assert (w >> 31).all()  # every record starts a read
    # runs of 1..6 equal ids, ids rising by 1 or more (and from a non-zero first id)
    runs = rng.integers(1, 7, 300)
    ids = np.repeat(5 + np.cumsum(rng.integers(1, 4, 300)), runs)
    rec = np.stack([ids, rng.integers(0, 500, len(ids))], 1).astype(np.uint32)
    w = check(rec)
    assert int((w >> 31).sum()) == 300
    assert np.array_equal(np.flatnonzero(w >> 31), np.r_[0, np.cumsum(runs)[:-1]])
    # the largest read id, and read ids that differ only in their top bit
    check([(0x7FFFFFFF, 1), (0x7FFFFFFF, 2), (0xFFFFFFFF, 3), (0xFFFFFFFF, 3)])


def test_contig_id_limit():
    top = (1 << 31) - 1
    assert check([(0, top), (0, 0), (1, top)]).tolist() == [0xFFFFFFFF, 0, 0xFFFFFFFF]
    for bad in ([(0, 1 << 31)], [(0, 1), (0, 1 << 31)], [(0, 1), (1, 0xFFFFFFFF)]):
        with pytest.raises(ValueError):
            engine.flag_records(np.array(bad, np.int64))
        with pytest.raises(ValueError):
            engine.flag_records(np.array(bad, np.uint32))


def test_ungrouped_read_ids_raise():
    # A, B, A with A > B at the repeat: three reads in the flagged format
    with pytest.raises(ValueError):
        engine.flag_records([(9, 1), (4, 2), (9, 3)])
    # ... and every other decrease, wherever it is
    for bad in ([(1, 0), (0, 0)], [(0, 0), (5, 1), (5, 2), (4, 3)], [(0, 0), (2, 1), (1, 2), (3, 3)],
                [(0xFFFFFFFF, 0), (0x7FFFFFFF, 0)]):
        with pytest.raises(ValueError):
            engine.flag_records(np.array(bad, np.uint32))
        with pytest.raises(ValueError):
            engine.flag_records(bad)
    # the pairs path accepts what does not decrease: so does this
    check([(4, 2), (9, 1), (9, 3)])
    rng = np.random.default_rng(1)
    rec = np.stack([np.sort(rng.integers(0, 300, 2000)), rng.integers(0, 100, 2000)], 1).astype(np.uint32)
    check(rec)
    rec[1500, 0] = rec[1499, 0] - 1  # one decrease in the middle
    with pytest.raises(ValueError):
        engine.flag_records(rec)


def test_list_strided_and_int64_inputs_give_the_same_words():
    rng = np.random.default_rng(2)
    ids = np.repeat(np.arange(400), rng.integers(1, 5, 400))
    rec = np.stack([ids, rng.integers(0, 1 << 20, len(ids))], 1).astype(np.uint32)
    w = check(rec)
    assert np.array_equal(engine.flag_records(rec.tolist()), w)
    assert np.array_equal(engine.flag_records(rec.astype(np.int64)), w)
    wide = np.zeros((len(rec), 5), np.uint32)  # columns 1 and 3 of a wider array
    wide[:, 1], wide[:, 3] = rec[:, 0], rec[:, 1]
    view = wide[:, 1::2]
    assert not view.flags["C_CONTIGUOUS"]
    assert np.array_equal(engine.flag_records(view), w)
    rows = np.repeat(rec, 2, axis=0)[::2]  # every other row of a longer array
    assert not rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(engine.flag_records(rows), w)
    fortran = np.asfortranarray(rec)
    assert np.array_equal(engine.flag_records(fortran), w)
