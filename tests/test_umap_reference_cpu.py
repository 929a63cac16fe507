"""The numpy model of the device UMAP (tests/umap_reference.py) judged on its
own: the defined kexp / klog against numpy's, the graph against the dense
formula, karma_umap_ab (a host entry of the library) against scipy's
curve_fit, and the contract as a usable UMAP on three blobs.  No device code."""
import numpy as np
import pytest

import umap_reference as ref
from karma_amd import engine

U64 = np.uint64
TINY = 2.0 ** -1074  # the quantum of a subnormal result


def _exp_sample():
    rng = np.random.default_rng(101)
    return np.concatenate([
        rng.uniform(-745.0, 709.0, 200000), rng.uniform(-1.0, 1.0, 50000), rng.normal(size=50000) * 1e-8,
        [0.0, -0.0, 709.0, -745.0, -744.5, -708.4, -708.3, 1.0, -1.0, 0.5 * np.log(2.0), -0.5 * np.log(2.0)]])


def test_kexp_against_numpy():
    x = _exp_sample()
    got, want = ref.kexp(x), np.exp(x)
    # a subnormal result carries an absolute quantum of 2^-1074, not 53 bits: one quantum there
    err = np.abs(got - want)
    bound = np.maximum(1e-14 * want, TINY)
    print("kexp worst relative error over normal results:", (err / want)[want >= 2.0 ** -1022].max())
    assert (err <= bound).all()
    # the clamps are part of the definition: beyond them the value is the clamp's
    low = np.array([-745.0, -745.0001, -746.0, -1e3, -1e300, -np.inf])
    assert (ref.kexp(low).view(U64) == ref.kexp(np.array([-745.0])).view(U64)).all()
    assert ref.kexp(np.array([-745.0]))[0] == np.exp(-745.0) == TINY
    high = np.array([709.0, 709.5, 710.0, 1e300, np.inf])
    assert (ref.kexp(high).view(U64) == ref.kexp(np.array([709.0])).view(U64)).all()
    assert abs(ref.kexp(np.array([709.0]))[0] - np.exp(709.0)) <= 1e-14 * np.exp(709.0)
    assert ref.kexp(np.array([0.0]))[0] == 1.0


def _log_sample():
    rng = np.random.default_rng(102)
    root = 0.7071067811865476
    around = np.concatenate([np.nextafter(root, 0.0) * np.ones(1), [root], np.nextafter(root, 1.0) * np.ones(1)])
    scaled = (around[None, :] * 2.0 ** np.arange(-1070, 1020, 55)[:, None]).ravel()  # m on both sides of sqrt(1/2)
    return np.concatenate([
        np.exp(rng.uniform(-700.0, 700.0, 200000)), 1.0 + rng.normal(size=50000) * 1e-3, rng.uniform(0.5, 2.0, 50000),
        scaled, [TINY, 3 * TINY, 2.0 ** -1023, 2.0 ** -1022, np.finfo(np.float64).max, 1e300, 1.0, 2.0, 0.5]])


def test_klog_against_numpy():
    x = _log_sample()
    got, want = ref.klog(x), np.log(x)
    err = np.abs(got - want)
    nz = want != 0.0
    print("klog worst relative error:", (err[nz] / np.abs(want[nz])).max())
    assert (err <= 1e-14 * np.abs(want)).all()
    assert ref.klog(np.array([1.0]))[0] == 0.0


def test_scalar_and_array_versions_agree_bit_for_bit():
    x = _exp_sample()[::97]
    assert [ref.kexp1(float(v)) for v in x] == ref.kexp(x).tolist()
    x = _log_sample()[::97]
    assert [ref.klog1(float(v)) for v in x] == ref.klog(x).tolist()
    b = 0.79
    assert [ref.kpow1(float(v), b) for v in x[:500]] == ref.kpow(x[:500], b).tolist()
    assert abs(ref.kpow1(3.0, 0.5) - np.sqrt(3.0)) < 1e-15


def test_splitmix_and_init():
    assert ref.splitmix64(12345) == 0xF36CF1164265DD51
    y = ref.init_y(50, 3, 42)
    assert y.shape == (50, 3) and (y >= -10.0).all() and (y < 10.0).all()
    assert len(np.unique(y)) == 150 and abs(y.mean()) < 2.0
    assert np.array_equal(ref.init_y(50, 3, 42), y) and not np.array_equal(ref.init_y(50, 3, 43), y)


def _dense_graph(idx, dist, sigma, rho):
    n, k = idx.shape
    a = np.zeros((n, n))
    for i in range(n):
        for j in range(k):
            c = idx[i, j]
            if c == i:
                continue
            d = dist[i, j] - rho[i]
            a[i, c] = 1.0 if d <= 0.0 or sigma[i] == 0.0 else np.exp(-d / sigma[i])
    return a + a.T - a * a.T


@pytest.mark.parametrize("n,m,k", [(40, 5, 2), (60, 8, 7), (90, 30, 15)])
def test_graph_against_the_dense_formula(n, m, k):
    rng = np.random.default_rng(n)
    x, _ = ref.blobs(rng, n, m, 3)
    x[n - 6:n - 3] = x[:3]  # duplicate rows: zero distances, rho from a later entry
    idx, dist = ref.knn_lists(x, k)
    indptr, indices, weights, sigma, rho = ref.umap_graph(idx, dist)
    dense = _dense_graph(idx, dist, sigma, rho)
    got = np.zeros((n, n))
    for i in range(n):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert (np.diff(cols) > 0).all()  # ascending, no column twice
        got[i, cols] = weights[indptr[i]:indptr[i + 1]]
    assert indptr[0] == 0 and indptr[-1] == len(indices) == len(weights) <= 2 * n * k
    assert (weights > 0).all() and (weights <= 1.0).all()
    assert np.abs(got - dense).max() <= 1e-12
    assert ((got != 0) == (dense != 0)).all()
    assert np.array_equal(got.view(U64), got.T.copy().view(U64))  # symmetric bit for bit


def test_graph_of_identical_rows_uses_the_global_mean():
    n, k = 9, 4
    idx = np.tile(np.arange(k, dtype=np.int32), (n, 1))  # every list names rows 0 .. k - 1 at distance 0
    dist = np.zeros((n, k))
    indptr, indices, weights, sigma, rho = ref.umap_graph(idx, dist)
    assert (rho == 0.0).all() and (weights == 1.0).all()
    # psum never reaches log2(k) from memberships of 1.0 only when k - 1 (or k) > log2(k): sigma is bisected down
    assert (sigma >= 0.0).all() and np.isfinite(sigma).all()
    assert indptr[-1] == len(indices)


@pytest.mark.parametrize("spread,min_dist", [(1.0, 0.0), (1.0, 0.1), (1.0, 0.5), (2.0, 0.25)])
def test_ab_against_curve_fit(spread, min_dist):
    optimize = pytest.importorskip("scipy.optimize")
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = optimize.curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    got_a, got_b = engine.umap_ab(spread, min_dist)
    print(f"ab({spread}, {min_dist}): library {got_a!r} {got_b!r}  curve_fit {a!r} {b!r}")
    assert abs(got_a - a) <= 1e-6 * a and abs(got_b - b) <= 1e-6 * b


def test_ab_known_values_and_errors():
    a, b = engine.umap_ab(1.0, 0.0)
    assert abs(a - 1.9328084) < 1e-5 and abs(b - 0.79049497) < 1e-5
    a, b = engine.umap_ab()
    assert abs(a - 1.57694346) < 1e-5 and abs(b - 0.89506088) < 1e-5
    for bad in ((0.0, 0.1), (-1.0, 0.1), (1.0, -0.1), (np.nan, 0.1), (1.0, np.inf)):
        with pytest.raises(ValueError):
            engine.umap_ab(*bad)


def test_the_contract_is_a_usable_umap():
    """120 points, 3 blobs in 30 dimensions, k = 10, 100 epochs, dim 2, library init."""
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(7)
    x, labels = ref.blobs(rng, 120, 30, 3)
    idx, dist = ref.knn_lists(x, 10)
    indptr, indices, weights, _, _ = ref.umap_graph(idx, dist)
    a, b = engine.umap_ab(1.0, 0.1)
    y = ref.umap_layout(indptr, indices, weights, 2, a, b, 100, 42)
    assert np.isfinite(y).all()
    score = metrics.silhouette_score(y, labels)
    print("silhouette of the true labels in the model's layout:", score)
    assert score >= 0.5
