"""The numpy model of karma_mreach_mst (tests/mst_reference.py) pinned without
a GPU: its Prim and Kruskal forms give the same edges on tie-heavy inputs (the
tree under a strict total order does not depend on the algorithm), its core
distances are the neighbour model's last column, and its sorted weights are
scipy's minimum spanning tree's of the dense mutual-reachability matrix."""
import numpy as np
import pytest

import knn_reference
import mst_reference as ref

U64 = np.uint64


def _inputs():
    rng = np.random.default_rng(5)
    grid = np.stack(np.meshgrid(np.arange(9.0), np.arange(7.0)), -1).reshape(-1, 2)
    return {
        "blobs": (ref.blobs(rng, 150, 4, 5), 5),
        "grid": (grid, 4),
        "lattice": (knn_reference.tie_lattice()[:120], 6),
        "identical": (np.ones((40, 3)), 3),
        "pairs": (np.repeat(rng.normal(size=(30, 3)), 2, axis=0), 2),
        "euclidean": (rng.normal(size=(90, 2)), 1),
        "all_rows": (rng.integers(0, 3, (50, 2)).astype(np.float64), 50),
        "two": (np.array([[0.0, 1.0], [3.0, 5.0]]), 2),
    }


@pytest.mark.parametrize("name", sorted(_inputs()))
def test_prim_and_kruskal_agree(name):
    x, min_samples = _inputs()[name]
    n = len(x)
    pa, pb, pw, pc = ref.mreach_mst(x, min_samples, ref.prim)
    ka, kb, kw, kc = ref.mreach_mst(x, min_samples, ref.kruskal)
    assert len(pa) == n - 1 and (pa < pb).all()
    assert np.array_equal(pa, ka) and np.array_equal(pb, kb)
    assert np.array_equal(pw.view(U64), kw.view(U64)) and np.array_equal(pc.view(U64), kc.view(U64))
    # ascending by (mr2, lo, hi); the rounded roots cannot decrease either
    assert (np.diff(pw) >= 0).all()
    # a spanning tree: n - 1 edges that join everything
    up = list(range(n))

    def find(v):
        while up[v] != v:
            v = up[v]
        return v

    for i, j in zip(pa, pb):
        assert find(i) != find(j)
        up[find(i)] = find(j)
    # core is the neighbour model's last distance, the row itself counted
    assert np.array_equal(pc.view(U64), knn_reference.knn(x, min_samples)[1][:, -1].view(U64))
    if min_samples == 1:
        assert (pc == 0).all()


def test_identical_rows_make_the_star_of_row_0():
    a, b, w, core = ref.mreach_mst(np.full((17, 2), 0.25), 4)
    assert (a == 0).all() and np.array_equal(b, np.arange(1, 17)) and (w == 0).all() and (core == 0).all()


@pytest.mark.parametrize("name", ["blobs", "grid", "lattice", "euclidean", "all_rows"])
def test_weights_are_scipys(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    x, min_samples = _inputs()[name]
    d2 = ref.d2_matrix(x)
    mr = np.sqrt(ref.mr2_matrix(d2, ref.core2_of(d2, min_samples)))
    upper = np.triu(mr, 1)
    assert (upper[np.triu_indices(len(x), 1)] > 0).all()  # scipy reads a zero as no edge: these inputs have none
    theirs = np.sort(csgraph.minimum_spanning_tree(upper).data)
    assert len(theirs) == len(x) - 1
    assert np.allclose(np.sort(ref.mreach_mst(x, min_samples)[2]), theirs, rtol=1e-12, atol=0)
