"""engine.mcl / DeviceAdj.mcl / ReadGraph.mcl on the GPU, bit for bit against
the numpy model (tests/mcl_reference.py): the matrix, the iteration count, the
chaos and the labels; the fused path against the general one; small batches;
early stops; device inputs, outputs and errors; and the text route end to end."""
from collections import OrderedDict

import numpy as np
import pytest

import mcl_reference as ref
from karma_amd import _lib, engine
from karma_amd.mcl import Mcl
from karma_amd.read_graph import ReadGraph

pytestmark = pytest.mark.gpu

RESOURCES = [2, 3, 4, 5, 8, 9, 32]
INFLATIONS = [2.0, 1.4, 6.0]


def _sizes():
    C = _lib.mcl_tile().COLS
    return sorted({1, 2, 3, C - 1, C, C + 1, 2 * C + 1})


def _bits(x):
    return np.float64(x).tobytes()


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _assert_result(got, want, what):
    for name, g, w in zip(("colptr", "rows", "vals"), got[:3], want[:3]):
        assert _same(g, w), (name, what)
    assert got[3] == want[3], ("iterations", what, got[3], want[3])
    assert _bits(got[4]) == _bits(want[4]), ("chaos", what, got[4], want[4])


def _check(graph, what, paths=(False, True), **kw):
    """Both paths against the model; the labels of the result against the model's."""
    want = ref.mcl(*graph, **kw)
    for general in paths:
        got = engine.mcl(*graph, general=general, **kw)
        _assert_result(got, want, (what, "general" if general else "default", kw))
        labels, count = engine.mcl_clusters(*got[:3])
        want_labels, want_count = ref.interpret(*want[:3])
        assert count == want_count and np.array_equal(labels, want_labels), (what, kw)
    return want


def _sparse(n, rng):
    """A random sparse graph: unsorted rows, input self-loops, and (n >= 3) an isolated last node."""
    edges = []
    last = n - 1 if n >= 3 else n
    for a in range(last):
        for b in range(a + 1, last):
            if rng.random() < min(1.0, 3.0 / n):
                edges.append((a, b, float(rng.uniform(0.05, 1.0))))
    edges += [(j, j, float(rng.uniform(0.05, 1.0))) for j in range(0, n, 3)]
    return ref.csr_from_edges(n, edges, rng)


def _star(n, hub=0, rng=None):
    """A hub joined to every other node, the others chained in pairs."""
    others = [j for j in range(n) if j != hub]
    edges = [(hub, j, 1.0) for j in others]
    edges += [(others[t], others[t + 1], 0.5) for t in range(0, len(others) - 1, 2)]
    return ref.csr_from_edges(n, edges, rng)


@pytest.mark.parametrize("resource", RESOURCES)
def test_sparse_graphs_equal_the_model_at_block_edges(resource):
    rng = np.random.default_rng(500 + resource)
    for n in _sizes():
        for inflation in INFLATIONS:
            _check(_sparse(n, rng), ("sparse", n), resource=resource, inflation=inflation)


@pytest.mark.parametrize("resource", RESOURCES)
def test_equal_weight_cliques_where_every_selection_is_a_tie(resource):
    C = _lib.mcl_tile().COLS
    for sizes, inflation in (([1, 2, 3, C - 1, C, C + 1], 2.0), ([5, 9, 2 * C + 1], 1.4), ([3, 7], 6.0)):
        edges, truth = ref.cliques(sizes)
        want = _check(ref.csr_from_edges(len(truth), edges), ("cliques", sizes), resource=resource,
                      inflation=inflation)
        assert want[3] == 1 and want[4] <= 2.0 ** -55
        labels, _ = ref.interpret(*want[:3])
        assert ref.pair_agreement(labels, truth) == 1.0


@pytest.mark.parametrize("resource", RESOURCES)
def test_star_whose_hub_spans_every_block(resource):
    C = _lib.mcl_tile().COLS
    rng = np.random.default_rng(520 + resource)
    for n, hub, inflation in ((2 * C + 1, 0, 2.0), (2 * C + 1, C, 1.4), (4 * C + 3, 4 * C + 2, 6.0)):
        _check(_star(n, hub, rng), ("star", n, hub), resource=resource, inflation=inflation)


def test_weighted_cliques_and_planted_groups_come_back():
    rng = np.random.default_rng(530)
    edges, truth = ref.cliques([1, 2, 3, 4, 5, 6, 9, 12, 20], rng)
    for resource, inflation in ((4, 2.0), (8, 1.4), (32, 6.0)):
        want = _check(ref.csr_from_edges(len(truth), edges, rng), "weighted cliques", resource=resource,
                      inflation=inflation)
        assert ref.pair_agreement(ref.interpret(*want[:3])[0], truth) == 1.0
    edges, truth = ref.planted(300, rng)
    want = _check(ref.csr_from_edges(300, edges, rng), "planted")
    assert ref.pair_agreement(ref.interpret(*want[:3])[0], truth) >= 0.99


def _batches(counts, cap):
    """The general path's batch rule (csrc/mcl_args.h), on the model's per-column candidate counts."""
    cap = max(cap, max(counts))
    bounds, j0 = [0], 0
    while j0 < len(counts):
        j1, total = j0 + 1, counts[j0]
        while j1 < len(counts) and total + counts[j1] <= cap:
            total += counts[j1]
            j1 += 1
        bounds.append(j1)
        j0 = j1
    return bounds


@pytest.mark.parametrize("resource", [4, 9])
def test_small_cand_cap_equals_the_default(resource):
    n, hub = 41, 20
    graph = _star(n, hub, np.random.default_rng(540))
    cols = ref.start(*graph)
    counts = [sum(len(cols[k]) for k, _ in col) for col in cols]
    assert counts[hub] == max(counts)
    for cap in (1, counts[hub] + 3, 2 * counts[hub]):
        bounds = _batches(counts, cap)
        assert len(bounds) - 1 >= 3
        if cap <= counts[hub] + 3:
            assert hub in bounds and hub + 1 in bounds  # batch edges on the wide column: it fills a batch alone
        want = ref.mcl(*graph, resource=resource)
        for general in (False, True):
            got = engine.mcl(*graph, resource=resource, general=general, cand_cap=cap)
            _assert_result(got, want, ("cand_cap", cap, general))
    # later iterations in batches too: at most R * R candidates per column, a cap of 40 cuts them up
    rng = np.random.default_rng(541)
    sparse = _sparse(60, rng)
    _assert_result(engine.mcl(*sparse, resource=resource, general=True, cand_cap=40),
                   ref.mcl(*sparse, resource=resource), "small cap, every iteration")


@pytest.mark.parametrize("max_iter", [1, 2, 3, 5, 6])
def test_early_stop_returns_the_matrix(max_iter):
    """Stops before convergence, at every place in the fused path's queue of launches."""
    rng = np.random.default_rng(550)
    edges, _ = ref.planted(70, rng)
    graph = ref.csr_from_edges(70, edges, rng)
    for resource in (4, 8, 9):
        want = _check(graph, ("early stop", max_iter), resource=resource, max_iter=max_iter)
        assert want[3] == max_iter and not want[4] < 1e-3
    # the singleton rule: a random graph on which a run stopped at 3 leaves a node naming no attractor
    rng = np.random.default_rng(11)
    edges = [(a, b, float(rng.uniform(0.05, 1))) for a in range(12) for b in range(a + 1, 12) if rng.random() < 0.3]
    want = _check(ref.csr_from_edges(12, edges), "no attractor", resource=2, max_iter=3)
    cols = ref.from_csc(*want[:3])
    att = {j for j, c in enumerate(cols) if any(i == j for i, _ in c)}
    assert any(not any(i in att for i, _ in c) for c in cols)


def test_eps_zero_runs_to_max_iter_and_large_eps_stops_at_once():
    graph = _sparse(20, np.random.default_rng(560))
    want = _check(graph, "eps 0", eps=0.0, max_iter=7)
    assert want[3] == 7 or want[4] < 0.0
    want = _check(graph, "eps 2", eps=2.0)
    assert want[3] == 1


def test_device_input_and_output():
    ctx = _lib.default_context()
    rng = np.random.default_rng(570)
    graph = _sparse(50, rng)
    want = ref.mcl(*graph)
    dev = [_lib.DevBuf.from_numpy(ctx, a) for a in graph]
    for general in (False, True):
        got = engine.mcl(*dev, general=general, out_device=True)
        assert all(isinstance(b, _lib.DevBuf) for b in got[:3])
        _assert_result((got[0].numpy(), got[1].numpy(), got[2].numpy(), got[3], got[4]), want, "device in and out")
        _assert_result(engine.mcl(*dev, general=general), want, "device in, host out")
        got = engine.mcl(*graph, general=general, out_device=True)
        _assert_result((got[0].numpy(), got[1].numpy(), got[2].numpy(), got[3], got[4]), want, "host in, device out")


def test_device_input_errors_return_normally():
    ctx = _lib.default_context()
    off = np.array([0, 2, 4, 6], np.int64)
    good = (off, np.array([1, 2, 0, 2, 0, 1], np.uint32), np.full(6, 0.5))
    bad = {"twice": (off, np.array([1, 1, 0, 2, 0, 1], np.uint32), good[2]),
           "outside": (off, np.array([1, 2, 0, 3, 0, 1], np.uint32), good[2]),
           "weights": (off, good[1], np.array([0.5, 0.5, 0.0, 0.5, 0.5, 0.5])),
           "off": (np.array([0, 4, 2, 6], np.int64), good[1], good[2])}
    for word, graph in bad.items():
        dev = [_lib.DevBuf.from_numpy(ctx, a) for a in graph]
        for general in (False, True):
            with pytest.raises(_lib.KarmaError) as e:
                engine.mcl(*dev, general=general)
            assert e.value.code == _lib.KARMA_ERR_ARG and word in str(e.value), (word, str(e.value))
    dev = [_lib.DevBuf.from_numpy(ctx, a) for a in good]
    _assert_result(engine.mcl(*dev), ref.mcl(*good), "after the errors")


@pytest.fixture(scope="module")
def eq_graph():
    """A ReadGraph of synthetic eq classes (300 contigs), as karma.py builds its full graph."""
    n = 300
    off, members, counts = engine.synth_eq_classes(9, n, 0, 4000, True)
    names = [f"ctg{i}" for i in range(n)]
    skip = np.zeros(len(counts), np.uint8)
    return ReadGraph._from_eq_arrays(names, off, members, counts, skip, OrderedDict((">" + x, "") for x in names))


def test_device_adj_route_equals_the_host_route(eq_graph):
    adj = eq_graph._device_mirror().adj
    _, off, nbr, w = adj.layout()
    assert off[-1] > 0
    for kw in (dict(), dict(resource=8, inflation=1.4), dict(resource=9), dict(general=True)):
        got = adj.mcl(**kw)
        _assert_result(got, engine.mcl(off, nbr, w, **kw), ("DeviceAdj.mcl", kw))
    _assert_result(adj.mcl(), ref.mcl(off, nbr, w), "DeviceAdj.mcl against the model")
    got = adj.mcl(out_device=True)
    _assert_result((got[0].numpy(), got[1].numpy(), got[2].numpy(), got[3], got[4]), ref.mcl(off, nbr, w),
                   "DeviceAdj.mcl, device out")


def test_text_routes_end_to_end(eq_graph):
    g = eq_graph
    text = g.mcl()
    assert text.endswith("\n") and Mcl(threads=4, inflation=2.0).run_pipe(g.edge_list()) == text
    lines = text.split("\n")[:-1]
    members = [line.split("\t") for line in lines]
    connected = set(g.get_connected_nodes())
    assert sorted(x for m in members for x in m) == sorted(connected)  # every node with an edge, once
    assert [len(m) for m in members] == sorted((len(m) for m in members), reverse=True)  # label order
    # the same clusters as the model's on the numbering the text defines
    from karma_amd.mcl import parse_abc

    names, off, nbr, w = parse_abc(g.edge_list())
    labels, count = ref.interpret(*ref.mcl(off, nbr, w)[:3])
    assert count == len(lines)
    assert members == [[names[j] for j in np.flatnonzero(labels == c)] for c in range(count)]
    # the consumers of the binary's stdout take the text unchanged
    sub = ReadGraph(g.subgraph(list(g.nodes())[:120]))
    sub_text = sub.mcl()
    assert Mcl(threads=1, inflation=2.0).run_pipe(sub.edge_list()) == sub_text
    original = list(sub.nodes())[:40]
    leftovers = sub.get_contigs_not_in_mcl_cluster_stdout(sub_text, original_contigs=original)
    kept = {x for c in sub.mcl_cluster for x in c}
    sub_connected = set(sub.get_connected_nodes())
    assert kept | set(leftovers) == sub_connected and not kept & set(leftovers)
    assert all(set(c) & set(original) for c in sub.mcl_cluster)
    sub.remove_nodes_from(leftovers)
    reps = sub.calculate_representative_sequences()
    assert len(reps) == len(sub.mcl_cluster) and all(r[1:] in c for r, c in zip(reps, sub.mcl_cluster))
    # another inflation is another text, from both routes alike
    assert Mcl(threads=1, inflation=1.4).run_pipe(sub.edge_list()) == sub.mcl(inflation=1.4)
