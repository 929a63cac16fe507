"""Pins tests/adj_reference.py (the model the device consumers are compared
with, tests/test_gpu_consumers_device.py) to networkx itself: seeded random
graphs of at most 60 nodes with self-loops, isolated nodes and shuffled
orders, built by add_nodes_from + add_edge, copied by nx.Graph(G.subgraph()),
trimmed by remove_nodes_from, and read with the reference's own expressions
(restated in test_gpu_consumers.py and test_gpu_rearrange.py).  No GPU calls."""
import random

import networkx as nx
import numpy as np
import pytest

import adj_reference as R
from test_gpu_consumers import ref_connected, ref_edge_list, ref_node_weights, ref_unconnected
from test_gpu_rearrange import ref_calc_connections

N_GRAPHS = 200


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_layout(got, want):
    return (all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and np.array_equal(bits(got[3]), bits(want[3]))
            and all(g.dtype == w.dtype for g, w in zip(got, want)))


def random_case(seed):
    """(node names by id, ids by position, a, b, w) of a simple graph with self-loops."""
    rng = random.Random(seed)
    n = rng.randint(1, 60)
    names = [f"n{seed}_{i}" if i % 3 else f"ν{i}" for i in range(n)]
    ids = list(range(n))
    rng.shuffle(ids)  # position -> name id
    pairs = [(i, j) for i in range(n) for j in range(i, n)]
    want = min(len(pairs), int(rng.choice([0, 0.5, 1, 2, 4]) * n))
    a, b, w = [], [], []
    for i, j in rng.sample(pairs, want):
        if rng.random() < 0.5:
            i, j = j, i
        a.append(i), b.append(j)
        w.append(rng.choice([rng.random(), rng.uniform(-1, 1) * 10.0 ** rng.randint(-30, 30), 0.5, 1e16]))
    return names, ids, a, b, w


def nx_graph(names, ids, a, b, w):
    G = nx.Graph()
    G.add_nodes_from(names[i] for i in ids)
    for x, y, z in zip(a, b, w):
        G.add_edge(names[ids[x]], names[ids[y]], weight=z)
    return G


def nx_layout(G, names):
    """The layout networkx itself holds: node order, adjacency-dict order, weights."""
    nid = {x: i for i, x in enumerate(names)}
    pos = {x: i for i, x in enumerate(G)}
    off, nbr, w = [0], [], []
    for u in G:
        for v, d in G.adj[u].items():
            nbr.append(pos[v])
            w.append(d["weight"])
        off.append(len(nbr))
    return (np.array([nid[x] for x in G], np.uint32), np.array(off, np.int64), np.array(nbr, np.uint32),
            np.array(w, np.float64))


def check_consumers(G, lay, names):
    """node_stats and edge_list of the model against the reference's expressions on G."""
    deg, nw = R.node_stats(lay)
    nodes = list(G)
    assert [x for x, d in zip(nodes, deg) if d == 0] == ref_unconnected(G)
    assert [x for x, d in zip(nodes, deg) if d != 0] == ref_connected(G)
    assert np.array_equal(deg, [len(G.adj[x]) for x in nodes])
    want = ref_node_weights(G)
    assert list(want) == nodes
    assert np.array_equal(bits(nw), bits([float(v) for v in want.values()]))
    assert R.edge_list(lay, names) == ref_edge_list(G)
    assert R.text_bytes(lay, names) == (len(ref_edge_list(G)) + 1 if G.number_of_edges() else 0)
    assert R.name_bytes(lay, names) == sum(len(x.encode()) for x in nodes)


@pytest.mark.parametrize("block", range(4))
def test_model_equals_networkx(block):
    for seed in range(1000 + block * N_GRAPHS // 4, 1000 + (block + 1) * N_GRAPHS // 4):
        names, ids, a, b, w = random_case(seed)
        rng = random.Random(seed + 7)
        G = nx_graph(names, ids, a, b, w)
        n = len(ids)
        lay = R.from_edges(n, a, b, w, ids)
        assert same_layout(lay, nx_layout(G, names)), seed
        check_consumers(G, lay, names)
        gpos = {x: i for i, x in enumerate(G)}
        # picks below half the nodes (networkx walks the filter set) and above (the graph's order)
        for frac in (0.0, 0.2, 0.45, 0.55, 0.8, 1.0):
            pick = rng.sample(list(G), int(frac * n))
            sg = nx.Graph(G.subgraph(pick))
            order = [gpos[x] for x in sg]  # the copy's own node order, as ReadGraph passes it
            vl = R.view(lay, order)
            assert same_layout(vl, nx_layout(sg, names)), (seed, frac)
            check_consumers(sg, vl, names)
            # remove_nodes_from on the copy, then a copy of what is left (three levels)
            drop = set(rng.sample(list(sg), rng.randint(0, len(sg)))) if len(sg) else set()
            mask = [x not in drop for x in sg]
            sg.remove_nodes_from(drop)
            kl = R.keep(vl, mask)
            assert same_layout(kl, nx_layout(sg, names)), (seed, frac, "keep")
            check_consumers(sg, kl, names)
            kpos = {x: i for i, x in enumerate(sg)}
            sg2 = nx.Graph(sg.subgraph(rng.sample(list(sg), len(sg) // 2 + len(sg) % 2)))
            vl2 = R.view(kl, [kpos[x] for x in sg2])
            assert same_layout(vl2, nx_layout(sg2, names)), (seed, frac, "view of keep")
            check_consumers(sg2, vl2, names)
        # remove_nodes_from on the built graph itself: only isolated nodes, then random ones
        iso = ref_unconnected(G)
        G.remove_nodes_from(iso)
        lay2 = R.keep(lay, [x not in set(iso) for x in gpos])
        assert same_layout(lay2, nx_layout(G, names)), (seed, "isolated")
        drop = set(rng.sample(list(G), len(G) // 3))
        mask = [x not in drop for x in G]
        G.remove_nodes_from(drop)
        assert same_layout(R.keep(lay2, mask), nx_layout(G, names)), (seed, "drop")


def ref_pair_walk(subs, G):
    """karma.py:103-118's walk, keeping what it sums: per (index_A, index_B) with
    an edge, the weight after the last product step and the number of edges."""
    import itertools

    out = []
    for ia, ib in itertools.combinations(subs, 2):
        weight, cnt = 0, 0
        for A, B in itertools.product(subs[ia]["mcl_subcluster"], subs[ib]["mcl_subcluster"]):
            if G.has_edge(A, B):
                weight += G[A][B]["weight"]
                cnt += 1
        if cnt:
            out.append((ia, ib, float(weight), cnt))
    return out


@pytest.mark.parametrize("block", range(2))
def test_cross_sums_equals_reference_walk(block):
    for seed in range(3000 + block * N_GRAPHS // 2, 3000 + (block + 1) * N_GRAPHS // 2):
        names, ids, a, b, w = random_case(seed)
        rng = random.Random(seed + 11)
        G = nx_graph(names, ids, a, b, w)
        lay = R.from_edges(len(ids), a, b, w, ids)
        nodes = list(G)
        rng.shuffle(nodes)
        left_out = rng.randint(0, len(nodes) // 4)  # nodes in no subcluster: sub = -1
        clustered, subs, i = nodes[left_out:], {}, 0
        while i < len(clustered):
            k = rng.randint(1, 6)
            subs[len(subs)] = {"previous_cluster": 1, "mcl_subcluster": clustered[i:i + k]}
            i += k
        gpos = {x: p for p, x in enumerate(G)}
        sub = np.full(len(gpos), -1, np.int64)
        rank = np.zeros(len(gpos), np.int64)
        for si, rec in subs.items():
            for r, x in enumerate(rec["mcl_subcluster"]):
                sub[gpos[x]], rank[gpos[x]] = si, r
        walk = ref_pair_walk(subs, G)
        for cutoff in (0, -0.5, 0.3, float("inf")):
            A, B, S, N, O = R.cross_sums(lay, sub, rank, cutoff)
            assert list(zip(A.tolist(), B.tolist())) == [(x[0], x[1]) for x in walk], seed
            assert np.array_equal(bits(S), bits([x[2] for x in walk])), seed
            assert N.tolist() == [x[3] for x in walk], seed
            groups = [[int(x), int(y)] for x, y, c in zip(A, B, O) for _ in range(c)]
            assert groups == ref_calc_connections(subs, G, cutoff), (seed, cutoff)
