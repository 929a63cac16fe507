"""The numpy model of karma_knn_rows (tests/knn_reference.py) pinned without a
GPU: against a scalar loop of the definition, against integer arithmetic
where every operation is exact, against scikit-learn's brute-force search
where no two distances are close, and the tie fixture's own claim."""
import numpy as np

import knn_reference as ref


def _scalar_knn(x, k, row_lo, row_hi):
    """The definition with Python floats (IEEE f64, one rounding per operation)."""
    n, m = x.shape
    idx, dist = [], []
    for i in range(row_lo, row_hi):
        keyed = []
        for j in range(n):
            acc = 0.0
            for c in range(m):
                t = float(x[i, c]) - float(x[j, c])
                acc = acc + t * t
            keyed.append((np.float64(acc).view(np.uint64).item(), j, acc))
        keyed.sort(key=lambda e: (e[0], e[1]))
        idx.append([e[1] for e in keyed[:k]])
        dist.append([np.sqrt(np.float64(e[2])) for e in keyed[:k]])
    return np.array(idx, np.int32), np.array(dist, np.float64)


def test_model_is_the_scalar_definition():
    rng = np.random.default_rng(11)
    cases = [(rng.random((23, 7)), 5, 0, 23), (rng.standard_normal((17, 1)) * 1e3, 17, 3, 11),
             (ref.profile_like(rng, 31, 12), 4, 0, 31), (ref.tie_lattice()[:40], 8, 5, 25),
             (np.round(rng.random((12, 3)) * 2) * 1e-170, 6, 0, 12)]  # d2 subnormal or 0
    for x, k, lo, hi in cases:
        gi, gd = ref.knn(x, k, lo, hi)
        wi, wd = _scalar_knn(x, k, lo, hi)
        assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == (hi - lo, k)
        assert np.array_equal(gi, wi)
        assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64))


def test_integer_exact_case():
    """Integer values below 2^20, 70 columns: every difference, square and sum
    is an integer below 2^53, so int64 arithmetic is the answer with no
    rounding anywhere and no tolerance."""
    rng = np.random.default_rng(3)
    n, m, k = 130, 70, 9
    xi = rng.integers(0, 1 << 20, (n, m), dtype=np.int64)
    xi[40] = xi[7]  # a duplicate row and equal distances to it
    xi[99] = xi[7]
    assert m * ((1 << 20) - 1) ** 2 < 1 << 53
    d2i = ((xi[:, None, :] - xi[None, :, :]) ** 2).sum(axis=2)
    d2 = ref.d2_rows(xi.astype(np.float64))
    assert np.array_equal(d2, d2i.astype(np.float64)) and np.array_equal(d2.astype(np.int64), d2i)
    want = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2i), axis=1)[:, :k]
    idx, dist = ref.knn(xi.astype(np.float64), k)
    assert np.array_equal(idx, want)
    assert idx[40, :3].tolist() == [7, 40, 99] and idx[99, :3].tolist() == [7, 40, 99]
    assert np.array_equal(dist.view(np.uint64), np.sqrt(np.take_along_axis(d2i, want, 1).astype(np.float64))
                          .view(np.uint64))


def test_indices_against_sklearn_where_gaps_are_wide():
    from sklearn.neighbors import NearestNeighbors

    rng = np.random.default_rng(7)
    n, m, k = 400, 1088, 15
    x = ref.profile_like(rng, n, m, 30, 900)
    d2 = ref.d2_rows(x)
    order = ref.order_rows(d2)
    first = np.take_along_axis(d2, order[:, :k + 1], axis=1)
    gap = ((first[:, 1:] - first[:, :-1]) / first[:, 1:]).min()
    print(f"smallest relative gap between consecutive d2 among the first {k + 1}: {gap:.3g}")
    # sklearn's distances carry a few ulp of error of their own (1e-16 relative); no order can flip across this gap
    assert gap > 1e-9
    idx, _ = ref.knn_from_d2(d2, order, k)
    sk = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(x).kneighbors(x, return_distance=False)
    assert np.array_equal(idx, sk)


def test_tie_fixture_has_ties_at_the_boundary():
    x = ref.tie_lattice()
    assert x.shape == (257, 9)
    d2 = ref.d2_rows(x)
    order = ref.order_rows(d2)
    srt = np.take_along_axis(d2, order, axis=1)
    tied = int(np.count_nonzero(srt[:, 7] == srt[:, 8]))
    print(f"rows whose 8th and 9th d2 are equal: {tied}")
    assert tied >= 100
    # and the model breaks them by index
    i = np.flatnonzero(srt[:, 7] == srt[:, 8])
    assert np.all(order[i, 7] < order[i, 8])
