"""numpy model of karma_knn_rows (include/karma.h): the definition the GPU
kernel must reproduce bit for bit.

d2(i, j) is accumulated over the columns in ascending order from +0.0 as
acc = acc + t * t with t = x[i, c] - x[j, c]: three IEEE round-to-nearest f64
operations per column, which is what numpy computes elementwise.  A row's list
is the k rows with the smallest (d2, j); d2 >= +0, so the u64 bit patterns
order the same way.  dist is sqrt(d2), correctly rounded.
"""
import numpy as np


def d2_rows(x, row_lo=0, row_hi=None):
    """float64[(row_hi - row_lo), n]: d2 of the query rows against every row."""
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    row_hi = n if row_hi is None else row_hi
    q = x[row_lo:row_hi]
    acc = np.zeros((len(q), n), np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for c in range(m):
            t = q[:, c, None] - x[None, :, c]
            acc = acc + t * t
    return acc


def order_rows(d2):
    """int64[rows, n]: every row's candidates by ascending (d2 bits, index)."""
    bits = np.ascontiguousarray(d2).view(np.uint64)
    idx = np.broadcast_to(np.arange(d2.shape[1], dtype=np.int64), d2.shape)
    return np.lexsort((idx, bits), axis=1)


def knn_from_d2(d2, order, k):
    idx = order[:, :k]
    with np.errstate(over="ignore", under="ignore"):
        dist = np.sqrt(np.take_along_axis(d2, idx, axis=1))
    return idx.astype(np.int32), dist


def knn(x, k, row_lo=0, row_hi=None):
    """(idx int32[rows, k], dist float64[rows, k]) of the model."""
    d2 = d2_rows(x, row_lo, row_hi)
    return knn_from_d2(d2, order_rows(d2), k)


def profile_like(rng, n, m, len_lo=30, len_hi=900):
    """Rows shaped like the k-mer profile: multinomial counts over m columns
    divided by a length."""
    lengths = rng.integers(len_lo, len_hi, n)
    rows = rng.multinomial(lengths, np.full(m, 1.0 / m))
    return rows / lengths[:, None].astype(np.float64)


def tie_lattice():
    """257 rows on a quarter-step lattice in 9 dimensions: most rows have equal
    d2 at the k = 8 boundary."""
    return np.random.default_rng(1).integers(0, 2, (257, 9)) / 4
