"""The model of the spectral start (tests/spectral_reference.py) against itself
on hand cases, and the condition on the GPU fixtures that lets the eigenvalue
comparison of tests/test_gpu_spectral.py detect a missed eigenvector."""
import math

import numpy as np
import pytest

import spectral_reference as sr
import umap_reference as ur


def test_components_on_hand_cases():
    # 0 - 2 - 4, 1 - 3, 5 alone; an entry in one direction joins as well
    indptr = np.array([0, 1, 1, 2, 3, 3, 3], np.int64)
    indices = np.array([2, 4, 1], np.int32)
    comp, count = sr.components(indptr, indices)
    assert comp.tolist() == [0, 1, 0, 1, 0, 5] and count == 3 and comp.dtype == np.int32
    comp, count = sr.components(*sr.path_graph(7)[:2])
    assert comp.tolist() == [0] * 7 and count == 1
    comp, count = sr.components(*sr.cliques_graph([1, 2, 3], 0)[:2])
    assert comp.tolist() == [0, 1, 1, 3, 3, 3] and count == 3


def test_degrees_and_operator_on_a_path():
    g = sr.path_graph(4)
    d, isd = sr.degrees(g[0], g[2])
    h = 1.0 / math.sqrt(2.0)
    assert d.tolist() == [1.0, 2.0, 2.0, 1.0] and isd.tolist() == [1.0, h, h, 1.0]
    x = np.array([[1.0, 0.0], [0.0, 1.0], [2.0, 0.0], [0.0, 3.0]])
    got = sr.apply(*g, x)
    want = np.array([[1.0 * (h * 0.0), 1.0 * (h * 1.0)],
                     [h * ((1.0 * 1.0) + (h * 2.0)), h * ((1.0 * 0.0) + (h * 0.0))],
                     [h * ((h * 0.0) + (1.0 * 0.0)), h * ((h * 1.0) + (1.0 * 3.0))],
                     [1.0 * (h * 2.0), 1.0 * (h * 0.0)]])
    assert got.tobytes() == want.tobytes()
    # sqrt(d) is the eigenvector of eigenvalue 1; the dense operator agrees with the in-order one
    dense, sqd = sr.dense_operator(*g)
    assert np.allclose(sr.apply(*g, sqd[:, None])[:, 0], sqd, rtol=0, atol=1e-15)
    assert np.allclose(dense @ x, got, rtol=0, atol=1e-15)


def test_operator_leaves_an_empty_row_at_zero():
    indptr = np.array([0, 1, 1, 2], np.int64)
    g = (indptr, np.array([2, 0], np.int32), np.array([0.5, 0.5]))
    out = sr.apply(*g, np.ones((3, 2)))
    assert out[1].tolist() == [0.0, 0.0] and np.isfinite(out).all()


def test_path_spectrum_is_the_cosines():
    n = 12
    lam = sr.component_spectra(*sr.path_graph(n), n - 1)[0]
    want = 1.0 - np.cos(np.pi * np.arange(1, n) / (n - 1))
    assert np.allclose(lam, want, rtol=0, atol=1e-13)


def test_composition_on_hand_cases():
    seed, dim = 42, 2
    # one connected component: centred at 0, the largest entry on the box's edge
    vec = np.array([[0.5, -0.1], [-0.25, 0.7], [0.1, 0.2]])
    comp = np.zeros(3, np.int32)
    y = sr.compose(vec, comp, seed)
    noise = np.array([[1e-4 * (-1.0 + 2.0 * sr.unit(seed + 1, i, c, dim)) for c in range(dim)] for i in range(3)])
    assert np.abs(noise).max() <= 1e-4
    assert y.tobytes() == ((0.0 + (10.0 / 0.7) * vec) + noise).tobytes()
    # the start formula is karma_umap_layout's
    assert sr.random_start(5, 3, 7).tobytes() == ur.init_y(5, 3, 7).tobytes()
    # two components, one of a single vertex: its row is the centre and the noise; a failed one takes the random start
    comp = np.array([0, 0, 2], np.int32)
    vec = np.array([[0.6, 0.0], [-0.8, 0.0], [0.0, 0.0]])
    y = sr.compose(vec, comp, seed)
    share = 1.0 / 3.0
    centre = [(-10.0 + 20.0 * sr.unit(seed, 2, c, dim)) * (1.0 - share) for c in range(dim)]
    assert y[2].tolist() == [centre[c] + 1e-4 * (-1.0 + 2.0 * sr.unit(seed + 1, 2, c, dim)) for c in range(dim)]
    radius = 10.0 * ur.kpow1(2.0 / 3.0, 0.5)
    assert abs(radius - 10.0 * math.sqrt(2.0 / 3.0)) < 1e-13
    c0 = (-10.0 + 20.0 * sr.unit(seed, 0, 0, dim)) * (1.0 - 2.0 / 3.0)
    assert y[1, 0] == (c0 + (radius / 0.8) * -0.8) + 1e-4 * (-1.0 + 2.0 * sr.unit(seed + 1, 1, 0, dim))
    failed = sr.compose(vec, comp, seed, failed=(0,))
    assert failed[:2].tobytes() == ur.init_y(3, dim, seed)[:2].tobytes() and failed[2].tobytes() == y[2].tobytes()
    # a seed at the top of the range wraps
    assert np.isfinite(sr.compose(vec, comp, 2 ** 64 - 1)).all()


@pytest.mark.parametrize("name", sr.SOLVER_FIXTURES)
def test_gpu_fixtures_have_separated_eigenvalues(name):
    """Neighbouring distinct eigenvalues among the first dim + 2 differ by more than 1e-6 in every component: a
    vector with residual r lies within r <= 2e-8 of an exact eigenvalue, so a solver that skipped one cannot match
    the reference's list within the tolerance."""
    g = sr.solver_fixture(name)
    comp, count = sr.components(g[0], g[1])
    assert count == sr.SOLVER_COMPONENTS[name]
    for root, lam in sr.component_spectra(*g, max(sr.SOLVER_DIMS) + 2).items():
        assert len(lam) == max(sr.SOLVER_DIMS) + 2 and lam[0] > 1e-6  # connected: one trivial eigenvalue only
        gaps = np.diff(lam)
        distinct = gaps[gaps > 1e-12]  # a cycle's eigenvalues come in exact pairs
        assert len(distinct) >= (len(gaps) if name != "cycle257" else len(gaps) // 2)
        assert distinct.min() > 1e-6, (name, root, distinct.min())
    # the weights are a valid input of the layout: symmetric, finite, in (0, 1]
    dense, _ = sr.dense_operator(*g)
    assert np.allclose(dense, dense.T, rtol=0, atol=1e-16) and g[2].min() > 0 and g[2].max() <= 1.0
