"""engine.hdbscan end to end on the GPU against the models
(tests/mst_reference.py, tests/hdbscan_tree_reference.py), and
KmerClustering.run(device_hdbscan=True): no `hdbscan` module anywhere, the
same cluster.txt and eval.txt as the model's labels give."""
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest

import hdbscan_tree_reference as tree_ref
import mst_reference as mst_ref
from karma_amd import _lib, engine
from karma_amd.kmer import KmerClustering

pytestmark = pytest.mark.gpu

U64 = np.uint64


def _model(x, min_cluster_size, min_samples, allow_single_cluster=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    a, b, w, _ = mst_ref.mreach_mst(x, min_samples)
    assert (w > 0).all()  # inside the tree's contract: no zero-weight edge
    return tree_ref.hdbscan_tree(a, b, w, len(x), min_cluster_size, allow_single_cluster)


@pytest.mark.parametrize("m", [2, 10])
def test_blobs_equal_the_model(m):
    rng = np.random.default_rng(50 + m)
    x = mst_ref.blobs(rng, 1500, m, 9, 0.08)
    x[1400:] = x[:100]  # duplicate rows, each twice: min_samples above that keeps every weight > 0
    for size, samples, single in ((5, None, False), (15, 4, False), (40, 3, True)):
        got = engine.hdbscan(x, size, samples, single)
        labels, prob = _model(x, size, size if samples is None else samples, single)
        assert got.labels_.dtype == np.int32 and got.probabilities_.dtype == np.float64
        assert np.array_equal(got.labels_, labels)
        assert np.array_equal(got.probabilities_.view(U64), prob.view(U64))
        assert labels.max() >= 2  # clusters were found


def test_one_row_and_tiny_inputs():
    got = engine.hdbscan(np.zeros((1, 3)), 2, 1)
    assert got.labels_.tolist() == [-1] and got.probabilities_.tolist() == [0.0]
    x = np.random.default_rng(60).normal(size=(9, 2))
    for single in (False, True):
        got = engine.hdbscan(x, 3, 2, single)
        labels, prob = _model(x, 3, 2, single)
        assert np.array_equal(got.labels_, labels) and np.array_equal(got.probabilities_.view(U64), prob.view(U64))


# ---- KmerClustering.run(device_hdbscan=True) -----------------------------------

@pytest.fixture(scope="module")
def seqs():
    blob, offs, _ = engine.synth_contigs(43, 500, 30, 900, 200)
    return OrderedDict((f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(500))


class _UMAP:
    def __init__(self, n_neighbors=15, n_components=2, min_dist=0.1, random_state=None):
        self.n_components = n_components

    def fit_transform(self, X):
        # a fixed linear map of the profile; float32, as umap-learn's embedding is
        X = np.asarray(X)
        axes = np.random.default_rng(44).normal(size=(X.shape[1], self.n_components))
        return (100.0 * X @ axes).astype(np.float32)


class _ModelHDBSCAN:
    """Stands where hdbscan.HDBSCAN would, for the expected files only: the model's labels."""

    def __init__(self, min_cluster_size=5, allow_single_cluster=False):
        self.size, self.single = min_cluster_size, allow_single_cluster

    def fit(self, reduced):
        self.labels_, self.probabilities_ = _model(reduced, self.size, self.size, self.single)
        return self


def _run(seqs, out_dir, min_cluster_size, **kw):
    out_dir.mkdir()
    KmerClustering(seqs, str(out_dir), "5p6", 4).run(15, 10, 0.1, 42, min_cluster_size, **kw)
    return (out_dir / "cluster.txt").read_text(), (out_dir / "eval.txt").read_text()


@pytest.mark.parametrize("min_cluster_size", [5, 1])
def test_run_without_the_hdbscan_package(seqs, monkeypatch, tmp_path, min_cluster_size):
    monkeypatch.setitem(sys.modules, "umap", types.SimpleNamespace(UMAP=_UMAP))
    monkeypatch.setitem(sys.modules, "hdbscan", types.SimpleNamespace(HDBSCAN=_ModelHDBSCAN))
    want = _run(seqs, tmp_path / "model", min_cluster_size)

    monkeypatch.setitem(sys.modules, "hdbscan", None)  # any `import hdbscan` raises ImportError from here on
    got = _run(seqs, tmp_path / "device", min_cluster_size, device_hdbscan=True)
    assert got == want
    fields = dict(zip(*[line.split("\t") for line in got[1].splitlines()]))
    assert fields["min_cluster_size"] == str(min_cluster_size)
    lines = [line.split("\t") for line in got[0].splitlines()]  # the unlabeled names, then one cluster per line
    assert len(lines) - 1 == int(fields["no_groups"]) and len(lines[0]) == int(fields["unlabeled"])
    assert sum(map(len, lines)) == len(seqs)
    assert sys.modules["hdbscan"] is None

    # the default path is what it was: it needs the package
    with pytest.raises(ImportError, match="needs umap-learn and hdbscan"):
        _run(seqs, tmp_path / "default", min_cluster_size)
    monkeypatch.setitem(sys.modules, "umap", None)
    with pytest.raises(ImportError, match="device_hdbscan=True"):
        _run(seqs, tmp_path / "no_umap", min_cluster_size, device_hdbscan=True)
