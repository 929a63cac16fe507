"""The numpy model of the blockwise neighbour lists (tests/knn_block_reference.py)
pinned without a device: folding any partition of the rows, in any block
order, is knn_reference.knn of the whole matrix, bit for bit, and so is the
ring of a sharded profile."""
import numpy as np
import pytest

import knn_block_reference as blk
import knn_reference as ref

U64 = np.uint64


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(U64), want[1].view(U64))


def _data(name):
    rng = np.random.default_rng(3)
    if name == "uniform":
        return rng.random((90, 7)), 15
    if name == "profile_like":
        return ref.profile_like(rng, 75, 33), 15
    return ref.tie_lattice(), 8


def _partitions(n):
    rng = np.random.default_rng(n)
    yield [0, n]
    yield [0, 1, n - 1, n]
    yield [0] + sorted(rng.choice(np.arange(1, n), 6, replace=False).tolist()) + [n]
    yield [0, n // 3, n // 3, n]  # an empty block


@pytest.mark.parametrize("name", ["uniform", "profile_like", "tie_lattice"])
def test_any_partition_in_any_order_is_knn(name):
    x, k = _data(name)
    want = ref.knn(x, k)
    for cuts in _partitions(len(x)):
        nb = len(cuts) - 1
        orders = [list(range(nb)), list(range(nb))[::-1], np.random.default_rng(nb).permutation(nb).tolist()]
        for order in orders:
            _same(blk.fold(x, cuts, order, k), want)
    # a query range folds like the whole
    _same(blk.fold(x, [0, 10, len(x)], [1, 0], k, 5, 31), ref.knn(x, k, 5, 31))


def test_the_lattice_ties_at_the_boundary_across_blocks():
    """Group A of the GPU tests proves something only if rows of different
    blocks tie at the k boundary: for most rows of the lattice the k-th and
    (k+1)-th candidates have equal d2 and lie in different blocks of every
    cut the GPU tests use (pieces of 1, c-1, c, c+1 rows; c = 128 here, and
    any c up to 128 divides the 257 rows into at least 3 blocks)."""
    x, k = ref.tie_lattice(), 8
    d2 = ref.d2_rows(x)
    order = ref.order_rows(d2)
    kth, nxt = order[:, k - 1], order[:, k]
    tied = np.take_along_axis(d2, kth[:, None], 1) == np.take_along_axis(d2, nxt[:, None], 1)
    tied = tied[:, 0]
    assert tied.sum() >= 100
    # the boundary's tie group (every candidate with the k-th's d2): its lowest index inside the list and its
    # highest index outside lie in different blocks, so some block order offers the loser first
    same = d2 == np.take_along_axis(d2, kth[:, None], 1)
    rank_of = np.argsort(order, axis=1)
    n = len(x)
    ids = np.arange(n)[None, :]
    first_in = np.where(same & (rank_of < k), ids, n).min(axis=1)
    last_out = np.where(same & (rank_of >= k), ids, -1).max(axis=1)
    assert (first_in[tied] < last_out[tied]).all()
    for piece in (1, 127, 128, 129):
        cross = tied & (first_in // piece != last_out // piece)
        assert cross.sum() >= 20, piece
    # and an index-blind rule (an equal d2 never displaces) gives another answer when blocks come in descending order
    cuts = [0, 128, 256, 257]
    keys, idx = blk.empty(len(x), k)
    for b in (2, 1, 0):
        bits = np.ascontiguousarray(blk.d2_block(x, x[cuts[b]:cuts[b + 1]])).view(U64)
        for r in range(cuts[b], cuts[b + 1]):
            col = bits[:, r - cuts[b]]
            enter = col < keys[:, -1]  # the blind test
            for i in np.flatnonzero(enter):
                kk = np.append(keys[i], col[i])
                ii = np.append(idx[i].astype(np.int64), r)
                o = np.lexsort((ii, kk))[:k]
                keys[i], idx[i] = kk[o], ii[o]
    assert not np.array_equal(idx, ref.knn(x, k)[0])


def test_update_merge_finish_details():
    rng = np.random.default_rng(5)
    q, c = rng.random((4, 3)), rng.random((6, 3))
    k = 8
    keys, idx = blk.update(None, None, q, c, 100, k)
    assert (keys[:, 6:] == blk.NO_KEY).all() and (idx[:, 6:] == blk.NO_IDX).all()  # k > nc: empty slots last
    assert (keys[:, 1:] >= keys[:, :-1]).all()
    assert set(idx[0, :6].tolist()) == set(range(100, 106))
    i2, d2 = blk.finish(keys, idx)
    assert (i2[:, 6:] == -1).all() and np.isposinf(d2[:, 6:]).all() and np.isfinite(d2[:, :6]).all()
    # no candidates: the state as it is; empty lists from nothing
    k2, j2 = blk.update(keys, idx, q, c[:0], 0, k)
    assert np.array_equal(k2, keys) and np.array_equal(j2, idx)
    e = blk.update(None, None, q, c[:0], 0, k)
    assert (e[0] == blk.NO_KEY).all() and (e[1] == blk.NO_IDX).all()
    # merge of two halves is the update with both
    a = blk.update(None, None, q, c[:3], 100, k)
    b = blk.update(None, None, q, c[3:], 103, k)
    m = blk.merge(*a, *b)
    assert np.array_equal(m[0], keys) and np.array_equal(m[1], idx)
    # no columns: every d2 is +0, ties by index
    z = blk.update(None, None, np.zeros((2, 0)), np.zeros((5, 0)), 7, 3)
    assert (z[0] == 0).all() and z[1].tolist() == [[7, 8, 9]] * 2


@pytest.mark.parametrize("bounds", [[0, 40, 90], [0, 0, 3, 50, 50, 90], [0, 90], [0, 1, 2, 3, 4, 5, 6, 7, 90]])
def test_ring_is_knn_for_uneven_bounds(bounds):
    x, k = _data("uniform")
    want = ref.knn(x, k)
    parts = blk.ring(x, bounds, k)
    assert [len(p[0]) for p in parts] == np.diff(bounds).tolist()
    _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want)
