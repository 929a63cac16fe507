"""The numpy model of the device UMAP (include/karma.h: karma_umap_graph,
karma_umap_layout): the judge of every output bit.

kexp / klog / kpow are the library's defined functions: every step is one IEEE
f64 operation, so plain Python floats (scalar versions, for the layout's loops)
and elementwise numpy (array versions) give the same bits.  Nothing here calls
np.exp, np.log, ** or np.sum where the contract defines an order."""
import math

import numpy as np

LOG2E = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
SQRT_HALF = 0.7071067811865476
# 13!, 12!, ..., 0! as doubles (all exact)
_FACT = [float(math.factorial(d)) for d in range(13, -1, -1)]
_EXP_C = [1.0 / f for f in _FACT]  # the correctly rounded quotients
_LOG_C = [1.0 / float(d) for d in range(23, 0, -2)]  # 1/23, 1/21, ..., 1/1

GOLDEN = 0x9E3779B97F4A7C15
EDGE_MUL = 0xD1342543DE82EF95
M64 = (1 << 64) - 1
TWO_M53 = math.ldexp(1.0, -53)


def kexp1(x):
    """kexp of one Python float."""
    x = min(max(x, -745.0), 709.0)
    n = float(round(x * LOG2E))  # round half to even: rint
    r = (x - n * LN2_HI) - n * LN2_LO
    p = _EXP_C[0]
    for c in _EXP_C[1:]:
        p = p * r + c
    h = math.floor(n * 0.5)
    return _ldexp1(_ldexp1(p, int(h)), int(n - h))


def _ldexp1(p, e):
    try:
        return math.ldexp(p, e)
    except OverflowError:
        return math.inf


def klog1(x):
    """klog of one Python float, x > 0 finite."""
    m, e = math.frexp(x)
    if m < SQRT_HALF:
        m = m * 2.0
        e = e - 1
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = _LOG_C[0]
    for c in _LOG_C[1:]:
        p = p * z + c
    e = float(e)
    return e * LN2_HI + ((2.0 * s) * p + e * LN2_LO)


def kpow1(x, b):
    return kexp1(b * klog1(x))


def kexp(x):
    """kexp elementwise on a float64 array."""
    x = np.minimum(np.maximum(np.asarray(x, np.float64), -745.0), 709.0)
    n = np.rint(x * LOG2E)
    r = (x - n * LN2_HI) - n * LN2_LO
    p = np.full_like(r, _EXP_C[0])
    for c in _EXP_C[1:]:
        p = p * r + c
    h = np.floor(n * 0.5)
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.ldexp(p, h.astype(np.int32)), (n - h).astype(np.int32))


def klog(x):
    """klog elementwise on a float64 array of finite values > 0."""
    m, e = np.frexp(np.asarray(x, np.float64))
    low = m < SQRT_HALF
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = np.full_like(z, _LOG_C[0])
    for c in _LOG_C[1:]:
        p = p * z + c
    return e * LN2_HI + ((2.0 * s) * p + e * LN2_LO)


def kpow(x, b):
    return kexp(b * klog(x))


def splitmix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---- the fuzzy graph ---------------------------------------------------------------

def _row_psum(idx_row, dist_row, i, rho, mid):
    psum = 0.0
    for j in range(len(idx_row)):
        if idx_row[j] == i:
            continue
        d = dist_row[j] - rho
        psum = psum + (kexp1(-(d / mid)) if d > 0.0 else 1.0)
    return psum


def smooth_knn(idx, dist):
    """(sigma, rho) float64[n] of the neighbour lists."""
    n, k = idx.shape
    idx_l, dist_l = idx.tolist(), dist.tolist()
    target = math.log2(float(k))
    rho, row_sum = [0.0] * n, [0.0] * n
    for i in range(n):
        s = 0.0
        first = 0.0
        for j in range(k):
            s = s + dist_l[i][j]
            if first == 0.0 and dist_l[i][j] > 0.0:
                first = dist_l[i][j]
        rho[i], row_sum[i] = first, s
    total = 0.0
    for i in range(n):
        total = total + row_sum[i]
    global_mean = total / float(n * k)
    sigma = [0.0] * n
    for i in range(n):
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            psum = _row_psum(idx_l[i], dist_l[i], i, rho[i], mid)
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == math.inf else (lo + hi) / 2.0
        mean = row_sum[i] / float(k) if rho[i] > 0.0 else global_mean
        sigma[i] = max(mid, 1e-3 * mean)
    return np.array(sigma, np.float64), np.array(rho, np.float64)


def memberships(idx, dist, sigma, rho):
    """A dict (i, j) -> membership of the directed entries, self entries dropped."""
    n, k = idx.shape
    idx_l, dist_l = idx.tolist(), dist.tolist()
    out = {}
    for i in range(n):
        for j in range(k):
            c = idx_l[i][j]
            if c == i:
                continue
            d = dist_l[i][j] - float(rho[i])
            out[(i, c)] = 1.0 if (d <= 0.0 or sigma[i] == 0.0) else kexp1(-(d / float(sigma[i])))
    return out


def umap_graph(idx, dist):
    """(indptr int64[n+1], indices int32[nnz], weights float64[nnz], sigma, rho)."""
    idx = np.asarray(idx, np.int32)
    dist = np.asarray(dist, np.float64)
    n = idx.shape[0]
    sigma, rho = smooth_knn(idx, dist)
    a = memberships(idx, dist, sigma, rho)
    rows = [dict() for _ in range(n)]
    for (i, c), p in a.items():
        q = a.get((c, i), 0.0)
        w = (p + q) - p * q
        if w == 0.0:
            continue
        rows[i][c] = w
        if (c, i) not in a:
            rows[c][i] = (q + p) - q * p
    indptr = np.zeros(n + 1, np.int64)
    indices, weights = [], []
    for i in range(n):
        for c in sorted(rows[i]):
            indices.append(c)
            weights.append(rows[i][c])
        indptr[i + 1] = len(indices)
    return indptr, np.array(indices, np.int32), np.array(weights, np.float64), sigma, rho


# ---- the layout ----------------------------------------------------------------------

def init_y(n, dim, seed):
    y = np.empty((n, dim), np.float64)
    for i in range(n):
        for c in range(dim):
            u = splitmix64(seed + (i * dim + c + 1) * GOLDEN) >> 11
            y[i, c] = -10.0 + 20.0 * (float(u) * TWO_M53)
    return y


def _clip4(v):
    return 4.0 if v > 4.0 else (-4.0 if v < -4.0 else v)


def umap_layout(indptr, indices, weights, dim, a, b, n_epochs, seed, y=None, negative_sample_rate=5, gamma=1.0,
                initial_alpha=1.0):
    """The layout after n_epochs, float64[n, dim]; y=None: the library's start."""
    n = len(indptr) - 1
    ip, ix, w = [int(v) for v in indptr], [int(v) for v in indices], [float(v) for v in weights]
    nnz = len(ix)
    R = int(negative_sample_rate)
    a, b, gamma, initial_alpha = float(a), float(b), float(gamma), float(initial_alpha)
    old = (init_y(n, dim, seed) if y is None else np.array(y, np.float64).reshape(n, dim)).tolist()
    wmax = 0.0
    for v in w:
        wmax = v if v > wmax else wmax
    eps, eons, eonns, t = [0.0] * nnz, [math.inf] * nnz, [math.inf] * nnz, [0] * nnz
    for e in range(nnz):
        if w[e] >= wmax / float(n_epochs):
            eps[e] = wmax / w[e]
            eons[e] = eps[e]
            if R:
                eonns[e] = eps[e] / float(R)
    dims = range(dim)
    for ep in range(n_epochs):
        alpha = initial_alpha * (1.0 - float(ep) / float(n_epochs))
        fep = float(ep)
        new = [None] * n
        for i in range(n):
            cur = list(old[i])
            for e in range(ip[i], ip[i + 1]):
                if not eons[e] <= fep:
                    continue
                o = old[ix[e]]
                df = [cur[c] - o[c] for c in dims]
                d2 = 0.0
                for c in dims:
                    d2 = d2 + df[c] * df[c]
                if d2 > 0.0:
                    pb = kpow1(d2, b)
                    g = ((-2.0 * a * b) * (pb / d2)) / (a * pb + 1.0)
                    for c in dims:
                        cur[c] = cur[c] + _clip4(g * df[c]) * alpha
                eons[e] = eons[e] + eps[e]
                if R:
                    epns = eps[e] / float(R)
                    nneg = int((fep - eonns[e]) / epns)
                    base = seed ^ ((e * EDGE_MUL) & M64)
                    for _ in range(nneg):
                        kk = splitmix64(base + (t[e] + 1) * GOLDEN) % n
                        t[e] = (t[e] + 1) & 0xFFFFFFFF
                        o = old[kk]
                        df = [cur[c] - o[c] for c in dims]
                        d2 = 0.0
                        for c in dims:
                            d2 = d2 + df[c] * df[c]
                        if d2 > 0.0:
                            g = (2.0 * gamma * b) / ((0.001 + d2) * (a * kpow1(d2, b) + 1.0))
                            for c in dims:
                                cur[c] = cur[c] + _clip4(g * df[c]) * alpha
                    eonns[e] = eonns[e] + float(nneg) * epns
            new[i] = cur
        old = new
    return np.array(old, np.float64).reshape(n, dim)


def default_epochs(n):
    return 500 if n <= 10000 else 200


def blobs(rng, n, m, centres, scale=1.0, spread=10.0):
    """n rows around `centres` Gaussian centres in m dimensions; (x, labels)."""
    c = rng.normal(size=(centres, m)) * spread
    labels = np.arange(n) % centres
    return c[labels] + rng.normal(size=(n, m)) * scale, labels


def knn_lists(x, k):
    """Neighbour lists as karma_knn_rows defines them (tests/knn_reference.py has the full model): d2 column by
    column from +0.0, the k smallest (d2, index), dist = sqrt(d2)."""
    x = np.asarray(x, np.float64)
    n, m = x.shape
    d2 = np.zeros((n, n))
    for c in range(m):
        t = x[:, None, c] - x[None, :, c]
        d2 = d2 + t * t
    idx = np.empty((n, k), np.int32)
    for i in range(n):
        idx[i] = np.lexsort((np.arange(n), d2[i]))[:k]
    return idx, np.sqrt(np.take_along_axis(d2, idx.astype(np.int64), 1))
