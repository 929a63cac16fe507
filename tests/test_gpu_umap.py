"""engine.umap_graph / umap_layout / umap on the GPU, bit for bit against the
numpy model (tests/umap_reference.py) fed the same neighbour lists from
engine.knn_rows, and KmerClustering.run(device_umap=True, device_hdbscan=True)
with neither `umap` nor `hdbscan` importable."""
import sys
from collections import OrderedDict

import numpy as np
import pytest

import umap_reference as ref
from karma_amd import _lib, engine
from karma_amd.kmer import KmerClustering

pytestmark = pytest.mark.gpu

A, B = 1.5769436133749897, 0.8950607195982855  # umap_ab(1, 0.1); inputs of the layout, any finite pair would do


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _check_graph(x, k):
    x = np.ascontiguousarray(x, dtype=np.float64)
    idx, dist = engine.knn_rows(x, k)
    got = engine.umap_graph(idx, dist, with_sigma=True)
    want = ref.umap_graph(idx, dist)
    for name, g, w in zip(("indptr", "indices", "weights", "sigma", "rho"), got, want):
        assert _same(g, w), (name, x.shape, k)
    return idx, dist, want


# ---- the graph --------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3, 15, 64])
def test_graph_equals_the_model_at_block_edges(k):
    T = _lib.umap_tile()
    rng = np.random.default_rng(300 + k)
    for n in sorted({2, 3, k, k + 1, T - 1, T, T + 1, 2 * T + 1}):
        if k > n:
            continue
        _check_graph(rng.normal(size=(n, 6)), k)


def test_graph_of_tripled_rows_takes_rho_from_a_later_entry():
    rng = np.random.default_rng(310)
    x = np.repeat(rng.normal(size=(20, 4)), 3, axis=0)
    idx, dist, (_, _, weights, _, rho) = _check_graph(x, 5)
    assert (dist[:, :3] == 0.0).all() and (rho == dist[:, 3]).all() and (rho > 0).all()
    assert (weights == 1.0).any()


def test_graph_of_identical_rows_uses_the_global_mean():
    idx, dist, (indptr, indices, _, sigma, rho) = _check_graph(np.ones((20, 3)), 4)
    assert (dist == 0.0).all() and (rho == 0.0).all()
    assert (idx[4:] != np.arange(4, 20)[:, None]).all()  # rows >= k are not in their own list
    assert indptr[-1] == len(indices) > 0


def test_graph_with_a_hub_across_blocks():
    T = _lib.umap_tile()
    n = 2 * T + 1
    x = np.zeros((n, n - 1))
    centre = T  # in the middle block
    others = [i for i in range(n) if i != centre]
    x[others, np.arange(n - 1)] = 100.0  # pairwise 100 sqrt(2) apart, 100 from the centre
    idx, dist, (indptr, indices, _, _, _) = _check_graph(x, 2)
    assert (idx[others, 1] == centre).all()
    assert indptr[centre + 1] - indptr[centre] == n - 1  # the reverse list spans every block
    assert np.array_equal(indices[indptr[centre]:indptr[centre + 1]], np.array(others, np.int32))


def test_graph_with_widely_spread_distances():
    # distances over twelve decades: kexp's argument passes its -745 clamp, where the membership is 2^-1074
    rng = np.random.default_rng(320)
    x = np.cumsum(10.0 ** rng.uniform(-6, 6, size=(40, 1)), axis=0)
    _, _, (_, _, weights, _, _) = _check_graph(x, 6)
    assert weights.min() < 1e-300 and weights.max() == 1.0


def test_graph_on_device_lists_and_outputs():
    rng = np.random.default_rng(330)
    x = rng.normal(size=(150, 5))
    idx, dist = engine.knn_rows(x, 7, out_device=True)
    want = ref.umap_graph(idx.numpy(), dist.numpy())
    got = engine.umap_graph(idx, dist, out_device=True, with_sigma=True)
    for g, w in zip(got, want):
        assert _same(g.numpy(), w)
    bad = idx.numpy()
    bad[149, 6] = 150
    with pytest.raises(_lib.KarmaError, match="neighbour index outside"):
        engine.umap_graph(_lib.DevBuf.from_numpy(idx.ctx, bad), dist)


# ---- the layout -------------------------------------------------------------------

_GRAPHS = {}


def _model_graph(n):
    if n not in _GRAPHS:
        x, _ = ref.blobs(np.random.default_rng(400 + n), n, 5, 3)
        idx, dist = ref.knn_lists(x, min(n - 1, {3: 2, 17: 5}.get(n, 10)))
        _GRAPHS[n] = ref.umap_graph(idx, dist)[:3]
    return _GRAPHS[n]


def _check_layout(graph, dim, epochs, rate, seed, init=None, **kw):
    got = engine.umap_layout(graph, dim, A, B, epochs, seed, init=init, negative_sample_rate=rate, **kw)
    want = ref.umap_layout(*graph, dim, A, B, epochs, seed, y=init, negative_sample_rate=rate, **kw)
    assert _same(got, want), (len(graph[0]) - 1, dim, epochs, rate, seed)
    return got


@pytest.mark.parametrize("n", [3, 17])
def test_layout_equals_the_model_small(n):
    graph = _model_graph(n)
    for dim in (1, 2, 10, 16):
        for epochs in (1, 3, 11, 50):
            for rate in (0, 1, 5):
                _check_layout(graph, dim, epochs, rate, seed=dim * 1000 + epochs * 10 + rate)


@pytest.mark.parametrize("dim,epochs,rate", [(1, 50, 1), (2, 11, 5), (10, 3, 0), (16, 1, 5), (2, 50, 5)])
def test_layout_equals_the_model_across_blocks(dim, epochs, rate):
    _check_layout(_model_graph(_lib.umap_tile() + 1), dim, epochs, rate, seed=77)


def test_layout_with_weights_over_four_decades():
    n = 17
    cycle = [1.0, 0.5, 0.03, 1e-3, 1e-4]  # every epoch, every second, once (epoch 34 of 50), pruned, pruned
    rows = [[] for _ in range(n)]
    for i in range(n):
        j = (i + 1) % n
        rows[i].append((j, cycle[i % 5]))
        rows[j].append((i, cycle[i % 5]))
    indptr = np.zeros(n + 1, np.int64)
    indices, weights = [], []
    for i in range(n):
        for c, w in sorted(rows[i]):
            indices.append(c)
            weights.append(w)
        indptr[i + 1] = len(indices)
    graph = (indptr, np.array(indices, np.int32), np.array(weights))
    for rate in (0, 5):
        moved = _check_layout(graph, 2, 50, rate, seed=5)
        assert np.isfinite(moved).all()


def test_layout_from_a_caller_start():
    graph = _model_graph(17)
    rng = np.random.default_rng(410)
    init = rng.normal(size=(17, 3))
    init[9] = init[4]  # two vertices at identical coordinates: d2 == 0 both ways
    keep = init.copy()
    _check_layout(graph, 3, 11, 5, seed=3, init=init)
    assert np.array_equal(init, keep)  # a host start is not changed
    _check_layout(graph, 3, 11, 5, seed=3, init=init * 1e3)   # attraction clipped at +-4
    _check_layout(graph, 3, 11, 5, seed=3, init=init * 1e-3)  # repulsion clipped
    _check_layout(graph, 3, 11, 5, seed=3, init=np.zeros((17, 3)))  # every d2 == 0: nothing moves
    _check_layout(graph, 2, 7, 5, seed=3, gamma=2.5, initial_alpha=0.25)


def test_layout_of_three_points_samples_itself():
    for seed in range(4):
        _check_layout(_model_graph(3), 2, 50, 5, seed=seed)


def test_layout_host_and_device_and_seeds():
    ctx = _lib.default_context()
    graph = _model_graph(17)
    init = np.random.default_rng(420).normal(size=(17, 2))
    want = _check_layout(graph, 2, 11, 5, seed=8, init=init)
    dev_graph = tuple(_lib.DevBuf.from_numpy(ctx, g) for g in graph)
    y = _lib.DevBuf.from_numpy(ctx, init)
    out = engine.umap_layout(dev_graph, 2, A, B, 11, 8, init=y)
    assert out is y and _same(y.numpy(), want)
    assert _same(engine.umap_layout(dev_graph, 2, A, B, 11, 8, init=init), want)
    first = engine.umap_layout(graph, 2, A, B, 11, 8)
    assert _same(engine.umap_layout(graph, 2, A, B, 11, 8), first)
    assert _same(engine.umap_layout(dev_graph, 2, A, B, 11, 8), first)
    assert not _same(engine.umap_layout(graph, 2, A, B, 11, 9), first)
    # a device graph's contents are checked by the first kernel
    bad = graph[1].copy()
    bad[0] = 17
    with pytest.raises(_lib.KarmaError, match="column outside"):
        engine.umap_layout((dev_graph[0], _lib.DevBuf.from_numpy(ctx, bad), dev_graph[2]), 2, A, B, 11, 8)


# ---- end to end -------------------------------------------------------------------

def test_umap_equals_the_model_end_to_end():
    x, _ = ref.blobs(np.random.default_rng(500), 300, 40, 4)
    idx, dist = engine.knn_rows(x, 15)
    a, b = engine.umap_ab(1.0, 0.1)
    want = ref.umap_layout(*ref.umap_graph(idx, dist)[:3], 2, a, b, 20, 42)
    assert _same(engine.umap(x, n_epochs=20), want)
    assert _same(engine.umap(x, n_epochs=20, knn=(idx, dist)), want)
    assert engine.umap(x, 5, 3, n_epochs=3, random_state=None).shape == (300, 3)


@pytest.fixture(scope="module")
def seqs():
    blob, offs, _ = engine.synth_contigs(43, 500, 30, 900, 200)
    return OrderedDict((f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(500))


def test_device_profile_input_equals_the_host_input(seqs):
    dev, _, _ = engine.kmer_profile_device(seqs, "5p6")
    try:
        host = dev.numpy()
        got = engine.umap(dev, 15, 10, n_epochs=10)
    finally:
        dev.close()
    assert got.shape == (500, 10) and _same(got, engine.umap(host, 15, 10, n_epochs=10))


def test_run_with_neither_package(seqs, monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "umap", None)  # any `import umap` / `import hdbscan` raises ImportError
    monkeypatch.setitem(sys.modules, "hdbscan", None)
    out = tmp_path / "device"
    out.mkdir()
    KmerClustering(seqs, str(out), "5p6", 4).run(15, 10, 0.1, 42, 5, device_umap=True, device_hdbscan=True)
    lines = [line.split("\t") for line in (out / "cluster.txt").read_text().splitlines()]

    profile, _, _ = engine.kmer_profile(seqs, "5p6")
    labels = engine.hdbscan(engine.umap(profile, 15, 10, 0.1, random_state=42), min_cluster_size=5).labels_
    names = [f"ctg{i}" for i in range(500)]
    groups = {frozenset(n for n, l in zip(names, labels) if l == c) for c in set(labels.tolist()) if c != -1}
    assert {frozenset(line) for line in lines[1:]} == groups and len(lines) - 1 == len(groups)
    assert set(lines[0]) - {""} == {n for n, l in zip(names, labels) if l == -1}
    assert sum(len(set(line) - {""}) for line in lines) == 500
    assert sys.modules["umap"] is None and sys.modules["hdbscan"] is None

    # with device_umap alone the clustering still needs its package
    with pytest.raises(ImportError, match="device_umap=True"):
        other = tmp_path / "no_hdbscan"
        other.mkdir()
        KmerClustering(seqs, str(other), "5p6", 4).run(15, 10, 0.1, 42, 5, device_umap=True)
