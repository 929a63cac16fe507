"""numpy model of karma_mreach_mst (include/karma.h): the definition the GPU
kernels must reproduce bit for bit.

d2(i, j) is tests/knn_reference.py's (karma_knn_rows').  core2(i) is the
min_samples-th smallest (d2(i, j), j) over all j, row i counted.  mr2(i, j) =
max(d2(i, j), core2(i), core2(j)).  Every value is >= +0, so the u64 bit
patterns order as the values do.  The tree is the one minimum spanning tree of
the complete graph under the strict total order of (mr2 bits, lo, hi), lo =
min(i, j) < hi; it is written ascending by that key with w = sqrt(mr2).  Two
forms that must agree: Prim with that comparison (n steps of an n-wide
lexicographic argmin) and Kruskal over all pairs sorted by that key.
"""
import numpy as np

import knn_reference


def d2_matrix(x):
    return knn_reference.d2_rows(np.asarray(x, dtype=np.float64))


def core2_of(d2, min_samples):
    order = knn_reference.order_rows(d2)
    return np.take_along_axis(d2, order[:, min_samples - 1:min_samples], axis=1)[:, 0]


def mr2_matrix(d2, core2):
    # no NaN and no -0 among these values: the maximum of the values is the maximum of the bit patterns
    return np.maximum(np.maximum(d2, core2[:, None]), core2[None, :])


def _finish(mr2, lo, hi):
    """Edges ascending by (mr2 bits, lo, hi); w = sqrt(mr2)."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    v = mr2[lo, hi] if len(lo) else np.zeros(0)
    order = np.lexsort((hi, lo, np.ascontiguousarray(v).view(np.uint64)))
    with np.errstate(over="ignore", under="ignore"):
        w = np.sqrt(v[order])
    return lo[order].astype(np.int32), hi[order].astype(np.int32), w


def prim(mr2):
    """(a, b, w) of the tree, grown from row 0: every step takes the smallest
    (mr2 bits, lo, hi) among the edges that leave the tree."""
    n = len(mr2)
    bits = np.ascontiguousarray(mr2).view(np.uint64)
    ids = np.arange(n, dtype=np.int64)
    inside = np.zeros(n, bool)
    inside[0] = True
    key = bits[0].copy()           # the best edge from the tree to j: its key ...
    lo = np.minimum(0, ids)        # ... and its endpoints
    hi = np.maximum(0, ids)
    ea, eb = [], []
    for _ in range(n - 1):
        sel = ~inside
        sel &= key == key[sel].min()
        sel &= lo == lo[sel].min()
        sel &= hi == hi[sel].min()
        j = int(np.flatnonzero(sel)[0])
        ea.append(int(lo[j])), eb.append(int(hi[j]))
        inside[j] = True
        nk, nlo, nhi = bits[j], np.minimum(j, ids), np.maximum(j, ids)
        better = (nk < key) | ((nk == key) & ((nlo < lo) | ((nlo == lo) & (nhi < hi))))
        better &= ~inside
        key = np.where(better, nk, key)
        lo = np.where(better, nlo, lo)
        hi = np.where(better, nhi, hi)
    return _finish(mr2, ea, eb)


def kruskal(mr2):
    """(a, b, w) of the tree: all pairs in ascending (mr2 bits, lo, hi), an
    edge kept when it joins two components."""
    n = len(mr2)
    lo, hi = np.triu_indices(n, 1)
    order = np.lexsort((hi, lo, np.ascontiguousarray(mr2[lo, hi]).view(np.uint64)))
    up = list(range(n))

    def find(v):
        while up[v] != v:
            up[v] = up[up[v]]
            v = up[v]
        return v

    ea, eb = [], []
    for e in order:
        if len(ea) == n - 1:
            break
        i, j = int(lo[e]), int(hi[e])
        ri, rj = find(i), find(j)
        if ri != rj:
            up[ri] = rj
            ea.append(i), eb.append(j)
    return _finish(mr2, ea, eb)


def mreach_mst(x, min_samples, form=prim):
    """(a int32[n-1], b int32[n-1], w float64[n-1], core float64[n]) of the model."""
    d2 = d2_matrix(x)
    c2 = core2_of(d2, min_samples)
    a, b, w = form(mr2_matrix(d2, c2))
    with np.errstate(over="ignore", under="ignore"):
        return a, b, w, np.sqrt(c2)


def blobs(rng, n, m, centres, spread=0.05):
    """n rows around `centres` Gaussian centres in m dimensions."""
    c = rng.normal(size=(centres, m))
    return c[rng.integers(0, centres, n)] + spread * rng.normal(size=(n, m))
