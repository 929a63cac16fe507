"""Plain Python / numpy models of the adjacency layouts networkx produces and of
their consumers (no test in here).  Each function restates one rule written at
the top of karma_amd/csrc/consumers.hip; tests/test_adj_reference_cpu.py pins
all of them to networkx itself, and tests/test_gpu_consumers_device.py compares
the device with them.

A layout is (ids, off, nbr, w): `ids[u]` = name id of the node at position u,
`off[n + 1]` into `nbr` (neighbour positions) and `w` (float64 weights), per
node in adjacency-dict order.  The layout functions are numpy throughout
(stable sorts), so a 270,000-node graph is modelled in well under a second;
sums and text use Python floats, as the reference does.
"""
import numpy as np


def _layout(ids, off, nbr, w):
    return (np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(off, np.int64),
            np.ascontiguousarray(nbr, np.uint32), np.ascontiguousarray(w, np.float64))


def _segments(off, nodes):
    """Entry indices of `nodes`' adjacency lists, concatenated, and the index
    into `nodes` each one belongs to."""
    off = np.asarray(off, np.int64)
    nodes = np.asarray(nodes, np.int64)
    lens = off[nodes + 1] - off[nodes]
    start = np.zeros(len(nodes) + 1, np.int64)
    np.cumsum(lens, out=start[1:])
    owner = np.repeat(np.arange(len(nodes), dtype=np.int64), lens)
    idx = np.arange(start[-1], dtype=np.int64) - start[owner] + off[nodes][owner]
    return idx, owner


def from_edges(n, a, b, w, ids=None):
    """add_edge(a[e], b[e], weight=w[e]) for e = 0, 1, ... on n pre-added nodes:
    adj[u] holds u's incident edges in call order; a self-loop appears once.

    Precondition: each unordered pair {a[e], b[e]} appears at most once (the
    graph builder guarantees it); a repeated add_edge would update the weight
    in place instead of appending."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    w = np.asarray(w, np.float64)
    e = np.arange(len(a), dtype=np.int64)
    other = a != b
    u = np.concatenate([a, b[other]])
    v = np.concatenate([b, a[other]])
    ee = np.concatenate([e, e[other]])
    o = np.lexsort((ee, u))  # by node, then by call
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=n), out=off[1:])
    return _layout(np.arange(n) if ids is None else ids, off, v[o], w[ee[o]])


def view(layout, order):
    """nx.Graph(G.subgraph(nodes)) with the copy's node order `order` (positions
    of G): adj[u] = u's view neighbours that come before u by view position,
    in position order, then the rest (u itself included) in G.adj[u] order."""
    ids, off, nbr, w = layout
    order = np.asarray(order, np.int64)
    k = len(order)
    pos = np.full(len(ids), -1, np.int64)
    pos[order] = np.arange(k)
    idx, i = _segments(off, order)
    x = pos[nbr[idx]]
    inside = x >= 0
    idx, i, x = idx[inside], i[inside], x[inside]
    noff = np.zeros(k + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=k), out=noff[1:])
    r = np.arange(len(i), dtype=np.int64) - noff[i]  # place among u's view neighbours, G.adj[u] order
    key = np.where(x < i, x, k + r)
    o = np.lexsort((key, i))
    return _layout(ids[order], noff, x[o], w[idx[o]])


def keep(layout, mask):
    """G.remove_nodes_from(nodes whose mask is 0): every remaining order unchanged."""
    ids, off, nbr, w = layout
    m = np.asarray(mask) != 0
    new = np.cumsum(m) - 1
    u = np.repeat(np.arange(len(ids), dtype=np.int64), np.diff(off))
    stay = m[u] & m[nbr]
    noff = np.zeros(int(m.sum()) + 1, np.int64)
    np.cumsum(np.bincount(new[u[stay]], minlength=len(noff) - 1), out=noff[1:])
    return _layout(ids[m], noff, new[nbr[stay]], w[stay])


def node_stats(layout):
    """(degrees, node weights): len(G.adj[u]) and 0.0 + w_1 + w_2 + ... over
    G.adj[u] in order, with Python floats, left to right."""
    _, off, _, w = layout
    wl = w.tolist()
    out = np.zeros(len(off) - 1, np.float64)
    for u in range(len(off) - 1):
        s = 0.0
        for x in wl[off[u]:off[u + 1]]:
            s += x
        out[u] = s
    return np.diff(off), out


def edge_lines(layout, names):
    """One UTF-8 line per edge, each from its earlier end: for u in order, for v
    in G.adj[u] with pos(v) >= pos(u).  names[i] = str or bytes of name id i."""
    ids, off, nbr, w = layout
    nm = [x if isinstance(x, bytes) else str(x).encode("utf-8") for x in names]
    idl, nl, wl = ids.tolist(), nbr.tolist(), w.tolist()
    out = []
    for u in range(len(idl)):
        a = nm[idl[u]]
        for j in range(off[u], off[u + 1]):
            if nl[j] >= u:
                out.append(a + b" " + nm[idl[nl[j]]] + b" " + f"{wl[j]!r}".encode("ascii"))
    return out


def edge_list(layout, names):
    """"\\n".join(f"{name_u} {name_v} {w!r}" ...) as UTF-8 (ReadGraph.edge_list)."""
    return b"\n".join(edge_lines(layout, names))


def text_bytes(layout, names):
    """sum(len(line) + 1): what the one-launch summary holds against its text budget."""
    return sum(len(x) + 1 for x in edge_lines(layout, names))


def name_bytes(layout, names):
    """UTF-8 bytes of the names of the layout's nodes."""
    nm = [x if isinstance(x, bytes) else str(x).encode("utf-8") for x in names]
    return sum(len(nm[i]) for i in layout[0].tolist())


def cross_sums(layout, sub, rank, cutoff):
    """Per subcluster pair (A, B), 0 <= A < B, joined by an edge, in (A, B) order:
    the weights of the entries u -> v with sub[u] == A and sub[v] == B, sorted
    by (rank[u], rank[v]) (itertools.product(nodes_A, nodes_B) order) and
    summed left to right from 0.0; their number; and how many of the running
    sums were > cutoff.  Returns (A, B, sum, n_edges, n_over) arrays."""
    ids, off, nbr, w = layout
    sub = np.asarray(sub, np.int64)
    rank = np.asarray(rank, np.int64)
    u = np.repeat(np.arange(len(ids), dtype=np.int64), np.diff(off))
    v = nbr.astype(np.int64)
    sel = (sub[u] >= 0) & (sub[v] > sub[u])
    u, v, ww = u[sel], v[sel], w[sel]
    o = np.lexsort((rank[v], rank[u], sub[v], sub[u]))
    u, v, wl = u[o], v[o], ww[o].tolist()
    pa, pb = sub[u].tolist(), sub[v].tolist()
    A, B, S, N, O = [], [], [], [], []
    j = 0
    while j < len(wl):
        s, t, over = 0.0, j, 0
        while t < len(wl) and pa[t] == pa[j] and pb[t] == pb[j]:
            s += wl[t]
            over += s > cutoff
            t += 1
        A.append(pa[j]), B.append(pb[j]), S.append(s), N.append(t - j), O.append(over)
        j = t
    return (np.array(A, np.int64), np.array(B, np.int64), np.array(S, np.float64), np.array(N, np.int64),
            np.array(O, np.int64))
