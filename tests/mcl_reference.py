"""The numpy model of the MCL contract (include/karma.h): Python floats, explicit
in-order sums, one IEEE operation at a time.  The judge of karma_mcl and
karma_mcl_clusters; written from the contract, not from the kernels."""

import numpy as np

from umap_reference import kpow1


def start(off, nbr, w):
    """The start matrix as a list of columns, each a list of (row, value) by row."""
    n = len(off) - 1
    cols = []
    for j in range(n):
        ent = {}
        for e in range(int(off[j]), int(off[j + 1])):
            i = int(nbr[e])
            if i == j:
                continue
            if i in ent:
                raise ValueError(f"neighbour {i} twice in column {j}")
            ent[i] = float(w[e])
        ent[j] = max(ent.values()) if ent else 1.0
        s = 0.0
        for i in sorted(ent):
            s = s + ent[i]
        cols.append([(i, ent[i] / s) for i in sorted(ent)])
    return cols


def inflate(x, inflation):
    return x * x if inflation == 2.0 else float(kpow1(x, inflation))


def iterate(cols, resource, inflation, cutoff):
    """One iteration: (new columns, chaos, candidates formed)."""
    new, chaos, cand = [], None, 0
    for col in cols:
        X = {}
        for k, tkj in col:  # k ascending
            for i, tik in cols[k]:
                X[i] = X.get(i, 0.0) + tik * tkj
                cand += 1
        order = sorted(X, key=lambda i: (-X[i], i))
        kept = [order[0]] + [i for i in order[1:resource] if X[i] >= cutoff]
        kept.sort()
        s = 0.0
        for i in kept:
            s = s + X[i]
        y = [inflate(X[i] / s, inflation) for i in kept]
        s2 = 0.0
        for v in y:
            s2 = s2 + v
        z = [v / s2 for v in y]
        sq = 0.0
        for v in z:
            sq = sq + v * v
        c = max(z) - sq
        chaos = c if chaos is None or c > chaos else chaos
        new.append(list(zip(kept, z)))
    return new, chaos, cand


def to_csc(cols):
    colptr = np.zeros(len(cols) + 1, np.int64)
    colptr[1:] = np.cumsum([len(c) for c in cols])
    rows = np.array([i for c in cols for i, _ in c], np.uint32)
    vals = np.array([v for c in cols for _, v in c], np.float64)
    return colptr, rows, vals


def from_csc(colptr, rows, vals):
    return [[(int(rows[t]), float(vals[t])) for t in range(int(colptr[j]), int(colptr[j + 1]))]
            for j in range(len(colptr) - 1)]


def mcl(off, nbr, w, inflation=2.0, resource=4, cutoff=1 / 4000, eps=1e-3, max_iter=100, with_counts=False):
    """(colptr, rows, vals, iterations, chaos) as engine.mcl returns them
    (with_counts: also the candidates formed per iteration)."""
    cols = start(off, nbr, w)
    it, chaos, counts = 0, None, []
    while True:
        cols, chaos, cand = iterate(cols, int(resource), float(inflation), float(cutoff))
        counts.append(cand)
        it += 1
        if chaos < eps or it == max_iter:
            break
    out = to_csc(cols) + (it, chaos)
    return out + (counts,) if with_counts else out


def interpret(colptr, rows, vals):
    """(labels int32[n], n_clusters) of a final matrix."""
    cols = from_csc(colptr, rows, vals)
    n = len(cols)
    att = [any(i == j for i, _ in cols[j]) for j in range(n)]
    system = list(range(n))  # attractor -> smallest attractor of its system

    def find(a):
        while system[a] != a:
            a = system[a]
        return a

    for b in range(n):
        if att[b]:
            for a, _ in cols[b]:
                if att[a]:
                    ra, rb = find(a), find(b)
                    if ra != rb:
                        system[max(ra, rb)] = min(ra, rb)
    cluster = []
    for j in range(n):
        mass = {}
        for a, v in cols[j]:
            if att[a]:
                r = find(a)
                mass[r] = mass.get(r, 0.0) + v
        cluster.append(min(mass, key=lambda r: (-mass[r], r)) if mass else n + j)
    members = {}
    for j, c in enumerate(cluster):
        members.setdefault(c, []).append(j)
    ranked = sorted(members.values(), key=lambda m: (-len(m), m[0]))
    labels = np.empty(n, np.int32)
    for lab, m in enumerate(ranked):
        labels[m] = lab
    return labels, len(ranked)


# ---- graphs ---------------------------------------------------------------------------

def csr_from_edges(n, edges, rng=None):
    """Symmetric CSR of undirected (a, b, w) edges; rows shuffled when rng is given."""
    adj = [[] for _ in range(n)]
    for a, b, wt in edges:
        adj[a].append((b, wt))
        if a != b:
            adj[b].append((a, wt))
    if rng is not None:
        for row in adj:
            rng.shuffle(row)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in adj])
    nbr = np.array([b for r in adj for b, _ in r], np.uint32)
    w = np.array([wt for r in adj for _, wt in r], np.float64)
    return off, nbr, w


def cliques(sizes, rng=None):
    """Disjoint cliques; weights uniform in [0.5, 1] (rng) or all 1.0.  (edges, truth)."""
    edges, truth, base = [], [], 0
    for c, m in enumerate(sizes):
        for a in range(m):
            for b in range(a + 1, m):
                edges.append((base + a, base + b, float(rng.uniform(0.5, 1.0)) if rng is not None else 1.0))
        truth += [c] * m
        base += m
    return edges, np.array(truth)


def planted(n, rng):
    """Groups of 1 to 6 nodes, 0.9 edge density, weights in [0.2, 1], plus n / 5 cross edges of weight <= 0.05."""
    truth, edges, base, g = np.empty(n, np.int64), [], 0, 0
    while base < n:
        m = min(int(rng.integers(1, 7)), n - base)
        truth[base:base + m] = g
        for a in range(m):
            for b in range(a + 1, m):
                if rng.random() < 0.9:
                    edges.append((base + a, base + b, float(rng.uniform(0.2, 1.0))))
        base += m
        g += 1
    have = {(a, b) for a, b, _ in edges}
    added = 0
    while added < n // 5:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        a, b = min(a, b), max(a, b)
        if a == b or truth[a] == truth[b] or (a, b) in have:
            continue
        have.add((a, b))
        edges.append((a, b, float(rng.uniform(0.001, 0.05))))
        added += 1
    return edges, truth


def star_chain(n):
    """A hub (node 0) joined to every other node, the others chained in pairs (1-2, 3-4, ...)."""
    edges = [(0, i, 1.0) for i in range(1, n)]
    edges += [(i, i + 1, 0.5) for i in range(1, n - 1, 2)]
    return edges


def pair_agreement(labels, truth):
    """The share of node pairs on which two labelings agree (same / different cluster)."""
    n = len(labels)
    la = np.asarray(labels)[:, None] == np.asarray(labels)[None, :]
    tr = np.asarray(truth)[:, None] == np.asarray(truth)[None, :]
    iu = np.triu_indices(n, 1)
    return float(np.mean(la[iu] == tr[iu]))
