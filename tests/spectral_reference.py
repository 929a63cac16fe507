"""The numpy/scipy model of the device spectral start (include/karma.h:
karma_graph_components, karma_spectral_apply, karma_umap_spectral): the judge
of the exact parts -- components, d and isd, the operator with its in-order
sums, the composition of y from given vectors -- and, by dense
numpy.linalg.eigh per component, of the eigenvalues.  The fixtures of
tests/test_gpu_spectral.py are built here, so the CPU tests can look at them
without a device."""
import math

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

from umap_reference import GOLDEN, TWO_M53, blobs, kpow1, splitmix64


# ---- the exact parts -----------------------------------------------------------------

def components(indptr, indices):
    """(comp int32[n], n_comp): every vertex's smallest component member."""
    n = len(indptr) - 1
    a = csr_matrix((np.ones(len(indices)), np.asarray(indices), np.asarray(indptr)), shape=(n, n))
    count, lab = connected_components(a, directed=False)
    first = np.full(count, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab].astype(np.int32), int(count)


def degrees(indptr, weights):
    """(d, isd): the in-order row sums from +0.0 and 1.0 / sqrt(d)."""
    n = len(indptr) - 1
    w = [float(v) for v in weights]
    d = np.zeros(n)
    for i in range(n):
        s = 0.0
        for e in range(int(indptr[i]), int(indptr[i + 1])):
            s = s + w[e]
        d[i] = s
    with np.errstate(divide="ignore"):
        return d, 1.0 / np.sqrt(d)


def apply(indptr, indices, weights, x):
    """S x, each entry isd(i) * (the sum in CSR order from +0.0 of (w * isd(j)) * x[j, c])."""
    x = np.asarray(x, np.float64)
    _, isd = degrees(indptr, weights)
    coef = np.asarray(weights, np.float64) * isd[np.asarray(indices, np.int64)]
    out = np.zeros_like(x)
    for i in range(len(indptr) - 1):
        s = np.zeros(x.shape[1])
        for e in range(int(indptr[i]), int(indptr[i + 1])):
            s = s + coef[e] * x[int(indices[e])]
        if indptr[i + 1] > indptr[i]:
            out[i] = isd[i] * s
    return out


def unit(seed, i, c, dim):
    return float(splitmix64(seed + (i * dim + c + 1) * GOLDEN) >> 11) * TWO_M53


def random_start(n, dim, seed, rows=None):
    """karma_umap_layout's start (on the given rows)."""
    rows = range(n) if rows is None else rows
    return np.array([[-10.0 + 20.0 * unit(seed, int(i), c, dim) for c in range(dim)] for i in rows])


def compose(vec, comp, seed, failed=()):
    """y from the returned vectors and labels; failed: the roots of components that did not converge."""
    vec = np.asarray(vec, np.float64)
    n, dim = vec.shape
    y = np.empty((n, dim))
    for r in np.unique(comp):
        rows = np.flatnonzero(comp == r)
        s = len(rows)
        if int(r) in failed:
            y[rows] = random_start(n, dim, seed, rows)
            continue
        m = min(dim, s - 1)
        share = float(s) / float(n)
        radius = 10.0 * kpow1(share, 1.0 / float(dim))
        vmax = float(np.abs(vec[rows, :m]).max()) if m else 0.0
        for c in range(dim):
            centre = (-10.0 + 20.0 * unit(seed, int(r), c, dim)) * (1.0 - share)
            for i in rows:
                v = centre
                if c < m:
                    v = v + (radius / vmax) * float(vec[i, c])
                y[i, c] = v + 1e-4 * (-1.0 + 2.0 * unit(seed + 1, int(i), c, dim))
    return y


# ---- the judge of the eigenvalues ------------------------------------------------------

def dense_operator(indptr, indices, weights):
    n = len(indptr) - 1
    a = csr_matrix((np.asarray(weights, np.float64), np.asarray(indices), np.asarray(indptr)), shape=(n, n)).toarray()
    d = a.sum(axis=1)
    with np.errstate(divide="ignore"):
        isd = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    return isd[:, None] * a * isd[None, :], np.sqrt(d)


def component_spectra(indptr, indices, weights, count):
    """{root: the `count` smallest nontrivial eigenvalues 1 - theta of the component, ascending (fewer where the
    component has fewer than count + 1 vertices)}."""
    comp, _ = components(indptr, indices)
    s_all, _ = dense_operator(indptr, indices, weights)
    out = {}
    for r in np.unique(comp):
        rows = np.flatnonzero(comp == r)
        if len(rows) < 2:
            out[int(r)] = np.zeros(0)
            continue
        theta = np.linalg.eigvalsh(s_all[np.ix_(rows, rows)])[::-1]  # descending; theta[0] = 1, the trivial one
        out[int(r)] = (1.0 - theta[1:1 + count])
    return out


# ---- fixtures ------------------------------------------------------------------------------

def csr_from_pairs(n, pairs):
    """A symmetric CSR graph, rows ascending by column, from {(i, j): w} with i != j (both directions are written)."""
    rows = [dict() for _ in range(n)]
    for (i, j), w in pairs.items():
        rows[i][j] = w
        rows[j][i] = w
    indptr = np.zeros(n + 1, np.int64)
    indices, weights = [], []
    for i in range(n):
        for c in sorted(rows[i]):
            indices.append(c)
            weights.append(rows[i][c])
        indptr[i + 1] = len(indices)
    return indptr, np.array(indices, np.int32), np.array(weights, np.float64)


def path_graph(n):
    return csr_from_pairs(n, {(i, i + 1): 1.0 for i in range(n - 1)})


def cycle_graph(n):
    return csr_from_pairs(n, {(i, (i + 1) % n): 1.0 for i in range(n)})


def knn_graph(x, k):
    """A symmetric k-nearest-neighbour graph with weights in (0, 1] (an input like karma_umap_graph's, made with
    numpy alone): a_ij = exp(-(d_ij - d_i,1) / mean_i) over i's k neighbours, w = max(a_ij, a_ji)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    sq = (x * x).sum(axis=1)
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0))
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    dk = np.take_along_axis(d, idx, 1)
    a = np.exp(-(dk - dk[:, :1]) / dk.mean(axis=1, keepdims=True))
    pairs = {}
    for i in range(n):
        for j, w in zip(idx[i].tolist(), a[i].tolist()):
            key = (min(i, j), max(i, j))
            pairs[key] = max(pairs.get(key, 0.0), w)
    return csr_from_pairs(n, pairs)


def cliques_graph(sizes, seed):
    """Cliques of the given sizes with random weights in [0.5, 1.5), one after the other (a size of 1: an isolated
    vertex)."""
    rng = np.random.default_rng(seed)
    pairs, base = {}, 0
    for s in sizes:
        for i in range(s):
            for j in range(i + 1, s):
                pairs[(base + i, base + j)] = 0.5 + float(rng.random())
        base += s
    return csr_from_pairs(base, pairs)


_FIXTURES = {}


def solver_fixture(name):
    """The solver's graphs (tests/test_gpu_spectral.py), built once."""
    if name not in _FIXTURES:
        if name == "path300":
            g = path_graph(300)
        elif name == "cycle257":
            g = cycle_graph(257)
        elif name == "blobs600":
            g = knn_graph(blobs(np.random.default_rng(1500), 600, 30, 3)[0], 15)
        elif name == "blobs2000":
            g = knn_graph(blobs(np.random.default_rng(1501), 2000, 30, 8)[0], 15)
        elif name == "gauss1000":
            g = knn_graph(np.random.default_rng(1502).normal(size=(1000, 8)), 15)
        else:
            raise KeyError(name)
        _FIXTURES[name] = g
    return _FIXTURES[name]


SOLVER_FIXTURES = ("path300", "cycle257", "blobs600", "blobs2000", "gauss1000")
SOLVER_COMPONENTS = {"path300": 1, "cycle257": 1, "blobs600": 3, "blobs2000": 8, "gauss1000": 1}
SOLVER_DIMS = (1, 2, 10)


def assert_finite(*arrays):
    for a in arrays:
        assert np.isfinite(a).all()


def sqrt_d(indptr, weights):
    return np.array([math.sqrt(v) for v in degrees(indptr, weights)[0]])
