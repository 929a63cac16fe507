"""engine.graph_components / spectral_apply / umap_spectral on the GPU against the
model (tests/spectral_reference.py): components, the operator and the
composition of y bit for bit; the eigenvectors by their properties; and the
spectral start through engine.umap and KmerClustering.run."""
import sys
from collections import OrderedDict

import numpy as np
import pytest

import spectral_reference as sr
import umap_reference as ur
from karma_amd import _lib, engine
from karma_amd.kmer import KmerClustering

pytestmark = pytest.mark.gpu

TOL = 1e-8


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _device(graph):
    ctx = _lib.default_context()
    return tuple(_lib.DevBuf.from_numpy(ctx, g) for g in graph)


def _edges(more=()):
    """Sizes around the solver's tile and around the 256-thread blocks of the per-row kernels."""
    T = _lib.spectral_tile()[0]
    return sorted({T - 1, T, T + 1, 2 * T + 1, 255, 256, 257, *more})


# ---- components -------------------------------------------------------------------------

def _check_components(graph):
    want, count = sr.components(graph[0], graph[1])
    got, n_comp = engine.graph_components(graph)
    assert _same(got, want) and n_comp == count
    return want, count


def test_components_of_paths_at_tile_edges():
    for n in _edges():  # a path: the worst case for label propagation
        _, count = _check_components(sr.path_graph(n))
        assert count == 1
        # the same path with its vertices shuffled: hooks no longer point one way
        perm = np.random.default_rng(n).permutation(n)
        _check_components(sr.csr_from_pairs(n, {(int(perm[i]), int(perm[i + 1])): 1.0 for i in range(n - 1)}))


def test_components_of_a_star_isolated_vertices_and_one_way_entries():
    T = _lib.spectral_tile()[0]
    n = 2 * T + 1
    hub = T  # in the middle block
    _, count = _check_components(sr.csr_from_pairs(n, {(hub, j): 1.0 for j in range(n) if j != hub}))
    assert count == 1
    # no entries at all; a single vertex
    assert _check_components((np.zeros(n + 1, np.int64), np.zeros(0, np.int32)))[1] == n
    assert _check_components((np.zeros(2, np.int64), np.zeros(0, np.int32)))[1] == 1
    # cliques between isolated vertices
    _, count = _check_components(sr.cliques_graph([1, 3, 1, 1, 70, 2, 1], 3))
    assert count == 7
    # entries written in one direction only still join
    indptr = np.array([0, 1, 1, 2, 3, 3, 3], np.int64)
    comp, count = _check_components((indptr, np.array([2, 4, 1], np.int32)))
    assert comp.tolist() == [0, 1, 0, 1, 0, 5]


def test_components_of_two_blobs_and_device_arrays():
    x, _ = ur.blobs(np.random.default_rng(1400), 300, 20, 2)
    idx, dist = engine.knn_rows(x, 10)
    graph = engine.umap_graph(idx, dist)
    want, count = _check_components(graph)
    assert count == 2 and set(want.tolist()) == {0, 1}
    dev = _device(graph)
    comp, n_comp = engine.graph_components(dev, out_device=True)
    assert n_comp == 2 and _same(comp.numpy(), want)
    assert _same(engine.graph_components(dev)[0], want)
    assert _same(engine.graph_components(graph, out_device=True)[0].numpy(), want)
    # a device graph's contents are checked by the first kernel
    bad = graph[1].copy()
    bad[5] = 300
    with pytest.raises(_lib.KarmaError, match="column outside"):
        engine.graph_components((dev[0], _lib.DevBuf.from_numpy(dev[0].ctx, bad)))


# ---- the operator -----------------------------------------------------------------------

def _ragged_graph(n, seed):
    """Rows of length 0 and 1, a hub longer than a block, the rest random; symmetric, random weights."""
    rng = np.random.default_rng(seed)
    hub = n // 2
    pairs = {(min(hub, j), max(hub, j)): float(rng.random()) + 0.01 for j in range(2, n) if j != hub}
    for _ in range(2 * n):
        i, j = (int(v) for v in rng.integers(2, n, 2))
        if i != j:
            pairs[(min(i, j), max(i, j))] = float(rng.random()) + 0.01
    pairs[(1, 2)] = 0.75  # vertex 1: one entry; vertex 0: none
    return sr.csr_from_pairs(n, pairs)


@pytest.mark.parametrize("p", [1, 3, 16, 32])
def test_operator_equals_the_model(p):
    for n in _edges((600,)):  # 600: the hub's row is longer than a block
        graph = _ragged_graph(n, 1000 + n)
        assert graph[0][1] == 0 and graph[0][2] - graph[0][1] == 1
        assert np.diff(graph[0]).max() >= n - 3
        x = np.random.default_rng(p * 1000 + n).normal(size=(n, p))
        want = sr.apply(*graph, x)
        assert _same(engine.spectral_apply(graph, x), want), (n, p)
        assert (want[0] == 0.0).all() and not np.signbit(want[0]).any()
    assert _same(engine.spectral_apply(_device(graph), x), want)


# ---- the solver -------------------------------------------------------------------------

_SOLVED = {}


def _solve(name, dim):
    if (name, dim) not in _SOLVED:
        graph = sr.solver_fixture(name)
        _SOLVED[(name, dim)] = engine.umap_spectral(graph, dim, 11, tol=TOL, with_stats=True)
    return _SOLVED[(name, dim)]


def _check_solution(graph, dim, y, st, tol):
    n = len(graph[0]) - 1
    comp, count = sr.components(graph[0], graph[1])
    assert _same(st.comp, comp) and st.components == count and st.not_converged == 0
    assert 1 <= st.outer_rounds <= 100 and st.applications >= st.outer_rounds
    sr.assert_finite(y, st.vec, st.lam, st.res)
    sqd = sr.sqrt_d(graph[0], graph[2])
    sv = sr.apply(*graph, st.vec)
    spectra = sr.component_spectra(*graph, dim)
    for r in np.unique(comp):
        rows = np.flatnonzero(comp == r)
        m = min(dim, len(rows) - 1)
        v = st.vec[rows, :m]
        assert (st.vec[rows, m:] == 0.0).all() and not np.signbit(st.vec[rows, m:]).any()
        if m == 0:
            continue
        assert np.abs(v.T @ v - np.eye(m)).max() <= 1e-10
        assert np.abs(v.T @ sqd[rows]).max() <= 1e-10
        theta = 1.0 - st.lam[r, :m]
        resid = np.sqrt(((sv[rows, :m] - v * theta) ** 2).sum(axis=0))
        assert resid.max() <= 2 * tol, (int(r), resid.max())
        assert st.res[r, :m].max() <= tol
        assert np.abs(np.sort(st.lam[r, :m]) - spectra[int(r)][:m]).max() <= tol, int(r)
        assert (np.diff(st.lam[r, :m]) >= -tol).all()  # the c-th largest theta: lam ascending
        first = np.abs(v).argmax(axis=0)  # argmax takes the first of equals: first by vertex
        assert (v[first, np.arange(m)] > 0).all()
    others = np.setdiff1d(np.arange(n), np.unique(comp))
    assert (st.lam[others] == 0.0).all() and (st.res[others] == 0.0).all()
    assert _same(y, sr.compose(st.vec, st.comp, 11))


@pytest.mark.parametrize("dim", sr.SOLVER_DIMS)
@pytest.mark.parametrize("name", sr.SOLVER_FIXTURES)
def test_solver_finds_the_eigenvectors(name, dim):
    y, st = _solve(name, dim)
    _check_solution(sr.solver_fixture(name), dim, y, st, TOL)
    if sr.SOLVER_COMPONENTS[name] == 1:  # one connected graph is centred at 0: the box's edge is reached
        assert np.abs(y).max() <= 10.0 + 1e-4 and np.abs(y).max() >= 10.0 - 1e-4


@pytest.mark.parametrize("dim", [2, 10])
def test_small_components_beside_a_large_one(dim):
    p = dim + _lib.spectral_tile()[1]
    sizes = [1, 2, dim, dim + 1, dim + 2, p, p + 1, 1, 200]
    blocks = sr.cliques_graph(sizes[:-1], 40 + dim)
    big = sr.knn_graph(np.random.default_rng(41).normal(size=(200, 5)), 10)
    base = len(blocks[0]) - 1
    graph = (np.concatenate([blocks[0], blocks[0][-1] + big[0][1:]]),
             np.concatenate([blocks[1], big[1] + base]).astype(np.int32), np.concatenate([blocks[2], big[2]]))
    y, st = engine.umap_spectral(graph, dim, 11, tol=TOL, with_stats=True)
    assert st.components == len(sizes)
    _check_solution(graph, dim, y, st, TOL)


def test_composition_of_an_unconverged_component():
    graph = sr.solver_fixture("path300")
    y, st = engine.umap_spectral(graph, 2, 5, tol=TOL, max_outer=1, with_stats=True)
    assert st.not_converged == 1 and st.components == 1 and st.outer_rounds == 1
    assert st.res[0].max() > TOL and (st.res[1:] == 0.0).all()
    assert _same(y, sr.random_start(300, 2, 5)) and _same(y, sr.compose(st.vec, st.comp, 5, failed=(0,)))
    # beside converged ones: cliques settle in the first round, the path does not
    blocks = sr.cliques_graph([4, 1, 6], 50)
    base = len(blocks[0]) - 1
    both = (np.concatenate([blocks[0], blocks[0][-1] + graph[0][1:]]),
            np.concatenate([blocks[1], graph[1] + base]).astype(np.int32), np.concatenate([blocks[2], graph[2]]))
    y, st = engine.umap_spectral(both, 3, 5, tol=TOL, max_outer=1, with_stats=True)
    assert st.not_converged == 1 and st.components == 4
    assert _same(y, sr.compose(st.vec, st.comp, 5, failed=(base,)))
    assert _same(y[base:], sr.random_start(base + 300, 3, 5, range(base, base + 300)))


def test_two_calls_and_host_and_device_graphs_give_the_same_bytes():
    graph = sr.solver_fixture("blobs600")
    y, st = _solve("blobs600", 2)
    again, st2 = engine.umap_spectral(graph, 2, 11, tol=TOL, with_stats=True)
    dev_y, dev_st = engine.umap_spectral(_device(graph), 2, 11, tol=TOL, with_stats=True, out_device=True)
    for a, b, c in ((y, again, dev_y.numpy()), (st.vec, st2.vec, dev_st.vec.numpy()),
                    (st.lam, st2.lam, dev_st.lam.numpy()), (st.res, st2.res, dev_st.res.numpy()),
                    (st.comp, st2.comp, dev_st.comp.numpy())):
        assert _same(a, b) and _same(a, c)
    assert (st.outer_rounds, st.applications) == (st2.outer_rounds, st2.applications)
    assert _same(engine.umap_spectral(graph, 2, 11, tol=TOL), y)  # without the optional outputs
    assert not _same(engine.umap_spectral(graph, 2, 12, tol=TOL), y)


# ---- end to end -------------------------------------------------------------------------

def test_umap_from_a_spectral_start_end_to_end():
    x, _ = ur.blobs(np.random.default_rng(500), 300, 40, 4)
    idx, dist = engine.knn_rows(x, 15)
    graph = engine.umap_graph(idx, dist)
    a, b = engine.umap_ab(1.0, 0.1)
    start = engine.umap_spectral(graph, 2, 42)
    want = engine.umap_layout(graph, 2, a, b, 20, 42, init=start)
    assert _same(engine.umap(x, n_epochs=20, init="spectral"), want)
    assert _same(engine.umap(x, n_epochs=20, init="spectral", knn=(idx, dist)), want)
    assert not _same(engine.umap(x, n_epochs=20), want)
    assert _same(engine.umap(x, n_epochs=20, init="random"), engine.umap(x, n_epochs=20))


def test_run_with_a_spectral_start_and_neither_package(monkeypatch, tmp_path):
    blob, offs, _ = engine.synth_contigs(43, 500, 30, 900, 200)
    seqs = OrderedDict((f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(500))
    monkeypatch.setitem(sys.modules, "umap", None)  # any `import umap` / `import hdbscan` raises ImportError
    monkeypatch.setitem(sys.modules, "hdbscan", None)
    KmerClustering(seqs, str(tmp_path), "5p6", 4).run(15, 10, 0.1, 42, 5, device_umap=True, device_hdbscan=True,
                                                       umap_init="spectral")
    lines = [line.split("\t") for line in (tmp_path / "cluster.txt").read_text().splitlines()]

    profile, _, _ = engine.kmer_profile(seqs, "5p6")
    reduced = engine.umap(profile, 15, 10, 0.1, random_state=42, init="spectral")
    labels = engine.hdbscan(reduced, min_cluster_size=5).labels_
    names = [f"ctg{i}" for i in range(500)]
    groups = {frozenset(n for n, l in zip(names, labels) if l == c) for c in set(labels.tolist()) if c != -1}
    assert {frozenset(line) for line in lines[1:]} == groups and len(lines) - 1 == len(groups)
    assert sum(len(set(line) - {""}) for line in lines) == 500
    assert sys.modules["umap"] is None and sys.modules["hdbscan"] is None
