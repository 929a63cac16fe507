"""karma_hdbscan_tree without a device: the library's host tail of HDBSCAN
(csrc/hdbscan_tree.cpp) against the plain-Python model
(tests/hdbscan_tree_reference.py): labels equal, probabilities bit for bit;
both against scikit-learn's own make_single_linkage and tree_to_labels, fed the
same ordered edges, where that scikit-learn is installed; the edge checks; and
the stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hdbscan_tree_reference as tree_ref
import mst_reference as mst_ref
from karma_amd import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")
U64 = np.uint64


def _mst(x, min_samples):
    a, b, w, _ = mst_ref.mreach_mst(np.asarray(x, np.float64), min_samples)
    assert (w > 0).all()
    return a, b, w, len(x)


def _cases():
    """name -> (a, b, w, n, min_cluster_size, allow_single_cluster): the model's spanning trees of small inputs."""
    rng = np.random.default_rng(3)
    cases = {}
    cases["blobs_2d"] = _mst(mst_ref.blobs(rng, 600, 2, 6), 5) + (5, False)
    cases["blobs_10d"] = _mst(mst_ref.blobs(rng, 400, 10, 8, 0.2), 10) + (10, False)
    cases["blobs_size_2"] = _mst(mst_ref.blobs(rng, 300, 3, 12, 0.1), 2) + (2, False)
    cases["noise"] = _mst(rng.random((300, 2)), 4) + (7, False)
    line = np.cumsum(1.0 + np.arange(120) % 7 + rng.random(120))[:, None]
    cases["chain"] = _mst(line, 1) + (4, False)
    cases["star"] = _mst(np.vstack([np.zeros(39), np.diag(1.0 + np.arange(39))]), 1) + (3, False)
    grid = np.stack(np.meshgrid(np.arange(12.0), np.arange(9.0)), -1).reshape(-1, 2)
    cases["equal_weights"] = _mst(grid, 1) + (5, False)
    cases["equal_weights_single"] = _mst(grid, 1) + (5, True)
    one_blob = rng.normal(size=(200, 2))
    cases["one_blob"] = _mst(one_blob, 5) + (5, False)
    cases["one_blob_single"] = _mst(one_blob, 5) + (5, True)
    size = 6
    for n in (2, size - 1, size, 2 * size - 1, 2 * size):
        for single in (False, True):
            cases[f"n_{n}{'_single' if single else ''}"] = _mst(rng.normal(size=(n, 2)), min(n, 3)) + (size, single)
    return cases


CASES = _cases()


def _library(a, b, w, n, size, single):
    labels, prob = np.full(n, -7, np.int32), np.full(n, -7.0)
    count = ctypes.c_int32(-7)
    rc = _lib.load().karma_hdbscan_tree(n, _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), size, int(single),
                                        _lib.ptr(labels), _lib.ptr(prob), ctypes.byref(count))
    return rc, labels, prob, count.value


@pytest.mark.parametrize("name", sorted(CASES))
def test_library_equals_the_model(name):
    a, b, w, n, size, single = CASES[name]
    assert n <= 600
    want_labels, want_prob = tree_ref.hdbscan_tree(a, b, w, n, size, single)
    rc, labels, prob, count = _library(a, b, w, n, size, single)
    assert rc == _lib.KARMA_OK
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(prob.view(U64), want_prob.view(U64))
    assert count == want_labels.max() + 1
    got = engine.hdbscan_tree(a, b, w, n, size, single)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert np.array_equal(got[0], labels) and np.array_equal(got[1].view(U64), prob.view(U64))


def test_the_cases_cover_clusters_noise_and_the_lone_root():
    seen = {name: tree_ref.hdbscan_tree(*CASES[name])[0] for name in CASES}
    assert seen["blobs_2d"].max() >= 3 and (seen["blobs_2d"] == -1).any()
    assert seen["blobs_size_2"].max() >= 8
    assert (seen["one_blob"] == -1).all() or seen["one_blob"].max() >= 1
    assert seen["one_blob_single"].max() == 0 and (seen["one_blob_single"] == -1).any()
    assert (seen["n_2"] == -1).all() and (seen["n_2_single"] == 0).all()
    assert (seen["n_5"] == -1).all() and (seen["n_11"] == -1).all()


def test_one_point():
    empty_i, empty_w = np.zeros(0, np.int32), np.zeros(0)
    for single in (False, True):
        rc, labels, prob, count = _library(empty_i, empty_i, empty_w, 1, 5, single)
        assert rc == _lib.KARMA_OK and labels.tolist() == [-1] and prob.tolist() == [0.0] and count == 0
        labels, prob = engine.hdbscan_tree(empty_i, empty_i, empty_w, 1, 5, single)
        assert labels.tolist() == [-1] and prob.tolist() == [0.0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_scikit_learn(name):
    linkage = pytest.importorskip("sklearn.cluster._hdbscan._linkage")
    tree = pytest.importorskip("sklearn.cluster._hdbscan._tree")
    if not (hasattr(linkage, "make_single_linkage") and hasattr(linkage, "MST_edge_dtype")
            and hasattr(tree, "tree_to_labels")):
        pytest.skip("this scikit-learn has no make_single_linkage / tree_to_labels")
    a, b, w, n, size, single = CASES[name]
    edges = np.empty(n - 1, dtype=linkage.MST_edge_dtype)
    edges["current_node"], edges["next_node"], edges["distance"] = a, b, w
    labels, prob = tree.tree_to_labels(linkage.make_single_linkage(edges), min_cluster_size=size,
                                       allow_single_cluster=single)
    want_labels, want_prob = tree_ref.hdbscan_tree(a, b, w, n, size, single)
    assert np.array_equal(labels, want_labels)
    assert np.allclose(prob, want_prob, rtol=0, atol=1e-12)


def test_edge_errors():
    a, b, w = np.array([0, 1, 2], np.int32), np.array([1, 2, 3], np.int32), np.array([1.0, 2.0, 3.0])
    bad = [(a, b, w[::-1].copy()),                                  # weights decrease
           (a, b, np.array([1.0, np.nan, 3.0])),
           (a, b, np.array([-1.0, 2.0, 3.0])),
           (a, np.array([1, 2, 0], np.int32), w),                   # closes a cycle
           (a, np.array([1, 1, 3], np.int32), w),                   # a loop
           (a, np.array([1, 2, 4], np.int32), w),                   # endpoint out of range
           (np.array([0, -1, 2], np.int32), b, w)]
    for ea, eb, ew in bad:
        rc, labels, prob, count = _library(ea, eb, ew, 4, 2, False)
        assert rc == _lib.KARMA_ERR_ARG
        assert (labels == -7).all() and (prob == -7.0).all() and count == -7  # nothing was written
        with pytest.raises(_lib.KarmaError) as e:
            engine.hdbscan_tree(ea, eb, ew, 4, 2)
        assert e.value.code == _lib.KARMA_ERR_ARG and "karma_hdbscan_tree" in str(e.value)
    assert _library(a, b, w, 4, 1, False)[0] == _lib.KARMA_ERR_ARG       # min_cluster_size < 2
    assert _library(a, b, w, 0, 2, False)[0] == _lib.KARMA_ERR_ARG
    assert _lib.load().karma_hdbscan_tree(4, None, _lib.ptr(b), _lib.ptr(w), 2, 0, None, None, None) == \
        _lib.KARMA_ERR_ARG
    assert _library(a, b, w, 4, 2, False)[0] == _lib.KARMA_OK


def test_python_argument_errors():
    a, b, w = np.array([0, 1], np.int32), np.array([1, 2], np.int32), np.array([1.0, 2.0])
    for size in (1, 0, -3):
        with pytest.raises(ValueError):
            engine.hdbscan_tree(a, b, w, 3, size)
    with pytest.raises(ValueError):
        engine.hdbscan_tree(a, b, w, 4, 2)  # n - 1 edges are needed
    with pytest.raises(ValueError):
        engine.hdbscan_tree(a, b, w[:1], 3, 2)
    with pytest.raises(ValueError):
        engine.hdbscan_tree(a, b, w, 0, 2)


def test_abi_declares_the_entry():
    lib = _lib.load()
    assert "karma_hdbscan_tree" in _lib.EXPORTED and hasattr(lib, "karma_hdbscan_tree")
    assert len(lib.karma_hdbscan_tree.argtypes) == 9


def test_tree_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "hdbscan_tree_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "hdbscan_tree_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_tree_sources_are_host_only():
    for name in ("hdbscan_tree.h", "hdbscan_tree.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "karma_internal.h\"" not in text
