"""numpy model of the blockwise neighbour lists (include/karma.h:
karma_knn_block, karma_knn_merge, karma_knn_finish), built on
knn_reference.d2_rows: the definition the GPU must reproduce bit for bit.

A state is (keys uint64[nq, k], idx int32[nq, k]): per row the k smallest
(d2 bits, index) seen so far, ascending, empty slots (all-ones, INT32_MAX)
last.  update() concatenates the carried entries with one block's
(d2 bits, cand_base + r), sorts by np.lexsort((idx, bits)) and keeps the first
k: nothing in it depends on the order in which blocks arrive.
"""
import numpy as np

import knn_reference as ref

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_IDX = np.int32(0x7FFFFFFF)


def empty(nq, k):
    return np.full((nq, k), NO_KEY, np.uint64), np.full((nq, k), NO_IDX, np.int32)


def _smallest(keys, idx, k):
    """Per row the k smallest (key, idx) of the given columns."""
    order = np.lexsort((idx, keys), axis=1)[:, :k]
    return np.take_along_axis(keys, order, 1), np.take_along_axis(idx, order, 1)


def d2_block(q, c):
    """float64[nq, nc]: d2 of every query row against every candidate row."""
    q, c = np.asarray(q, np.float64), np.asarray(c, np.float64)
    nq = len(q)
    return ref.d2_rows(np.concatenate([q, c]), 0, nq)[:, nq:]


def update(keys, idx, q, c, cand_base, k):
    """The state after folding candidate rows c (indices cand_base + r) into
    the lists of query rows q.  keys / idx None: the lists start empty."""
    nq, nc = len(q), len(c)
    if keys is None:
        keys, idx = empty(nq, k)
    assert keys.shape == idx.shape == (nq, k)
    bits = np.ascontiguousarray(d2_block(q, c)).view(np.uint64).reshape(nq, nc)
    cidx = np.broadcast_to(np.arange(cand_base, cand_base + nc, dtype=np.int64), (nq, nc))
    assert cand_base >= 0 and cand_base + nc <= 2 ** 31 - 1
    all_k = np.concatenate([keys, bits], axis=1)
    all_i = np.concatenate([idx.astype(np.int64), cidx], axis=1)
    nk, ni = _smallest(all_k, all_i, k)
    return nk, ni.astype(np.int32)


def merge(keys, idx, keys_b, idx_b):
    k = keys.shape[1]
    nk, ni = _smallest(np.concatenate([keys, keys_b], axis=1), np.concatenate([idx, idx_b], axis=1).astype(np.int64), k)
    return nk, ni.astype(np.int32)


def finish(keys, idx):
    """(idx, dist): an empty slot comes out as (-1, +inf)."""
    hole = (keys == NO_KEY) & (idx == NO_IDX)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dist = np.sqrt(np.ascontiguousarray(keys).view(np.float64))
    return np.where(hole, np.int32(-1), idx).astype(np.int32), np.where(hole, np.inf, dist)


def fold(x, cuts, order, k, row_lo=0, row_hi=None):
    """knn of the rows [row_lo, row_hi) of x, folding the row blocks cut at
    `cuts` (ascending bounds from 0 to len(x)) in the given order."""
    row_hi = len(x) if row_hi is None else row_hi
    q = x[row_lo:row_hi]
    keys = idx = None
    for b in order:
        keys, idx = update(keys, idx, q, x[cuts[b]:cuts[b + 1]], cuts[b], k)
    return finish(keys, idx)


def ring(x, bounds, k):
    """Per rank (idx, dist) of its rows [bounds[r], bounds[r + 1]): round s
    folds the block that began at rank (r + s) % world."""
    world = len(bounds) - 1
    out = []
    for r in range(world):
        out.append(fold(x, bounds, [(r + s) % world for s in range(world)], k, bounds[r], bounds[r + 1]))
    return out
