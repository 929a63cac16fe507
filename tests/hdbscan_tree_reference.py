"""Plain-Python model of karma_hdbscan_tree (include/karma.h): from a spanning
tree's edges, in the order given, to HDBSCAN labels and probabilities.

Single linkage by a union-find over the edges; condensing breadth-first from
the root with lambda = 1 / w; stability; excess of mass from the deepest label
up; labels by ascending selected label; probabilities.  This is what
scikit-learn 1.7's make_single_linkage and tree_to_labels compute with their
defaults, written out anew.  All arithmetic is IEEE f64 in a fixed order, so the
library's probabilities must equal these bit for bit.
"""
import math

import numpy as np


def single_linkage(n, a, b, w):
    """Per merge e (node n + e): (left, right, w, size); left = find(a), right = find(b)."""
    up = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)

    def find(v):
        r = v
        while up[r] != r:
            r = up[r]
        while up[v] != r:
            up[v], v = r, up[v]
        return r

    merges = []
    for e in range(n - 1):
        if e and w[e] < w[e - 1]:
            raise ValueError("weights must not decrease")
        left, right = find(int(a[e])), find(int(b[e]))
        if left == right:
            raise ValueError("not a tree")
        size[n + e] = size[left] + size[right]
        up[left] = up[right] = n + e
        merges.append((left, right, float(w[e]), size[n + e]))
    return merges


def _breadth_first(n, merges, start):
    out = [start]
    head = 0
    while head < len(out):
        node = out[head]
        head += 1
        if node >= n:
            out += [merges[node - n][0], merges[node - n][1]]
    return out


def condense(n, merges, min_cluster_size):
    """Entries (parent label, child, lambda, size) in the order they are made; labels count from n (the root)."""
    root = 2 * n - 2
    label = {root: n}
    next_label = n + 1
    gone = set()
    entries = []
    count = lambda node: 1 if node < n else merges[node - n][3]  # noqa: E731

    def fall_out(start, parent, lam):
        for s in _breadth_first(n, merges, start):
            if s < n:
                entries.append((parent, s, lam, 1))
            gone.add(s)

    for node in _breadth_first(n, merges, root):
        if node < n or node in gone:
            continue
        left, right, dist, _ = merges[node - n]
        lam = 1.0 / dist if dist > 0.0 else math.inf
        lc, rc = count(left), count(right)
        here = label[node]
        if lc >= min_cluster_size and rc >= min_cluster_size:
            for side, c in ((left, lc), (right, rc)):
                label[side] = next_label
                entries.append((here, next_label, lam, c))
                next_label += 1
        else:
            for side, c in ((left, lc), (right, rc)):
                if c < min_cluster_size:
                    fall_out(side, here, lam)
                else:
                    label[side] = here
    return entries, next_label - n


def labels_from_condensed(n, entries, clusters, allow_single_cluster):
    birth = {n: 0.0}
    above = {}
    kids = {n + k: [] for k in range(clusters)}
    for parent, child, lam, _ in entries:
        if child >= n:
            birth[child] = lam
            above[child] = parent
            kids[parent].append(child)
    stability = {n + k: 0.0 for k in range(clusters)}
    top = {}
    for parent, child, lam, size in entries:
        stability[parent] += (lam - birth[parent]) * size
        top[parent] = lam if parent not in top else max(top[parent], lam)

    selected = {c: True for c in stability}
    if not allow_single_cluster:
        selected[n] = False
    for c in sorted(stability, reverse=True):
        if c == n and not allow_single_cluster:
            continue
        below = sum((stability[k] for k in kids[c]), 0.0)
        if below > stability[c]:
            selected[c] = False
            stability[c] = below
        else:
            todo = list(kids[c])
            while todo:
                s = todo.pop()
                selected[s] = False
                todo += kids[s]

    chosen = sorted(c for c in selected if selected[c])
    number = {c: k for k, c in enumerate(chosen)}
    lone_root = allow_single_cluster and chosen == [n]

    labels = np.full(n, -1, np.int32)
    prob = np.zeros(n, np.float64)
    for parent, child, lam, _ in entries:
        if child >= n:
            continue
        c = parent
        while not selected[c] and c != n:
            c = above[c]
        if not selected[c]:
            continue
        if c == n and not (lone_root and lam >= top[n]):
            continue
        labels[child] = number[c]
        prob[child] = 1.0 if top[c] == 0.0 or not math.isfinite(top[c]) else min(lam, top[c]) / top[c]
    return labels, prob


def hdbscan_tree(a, b, w, n, min_cluster_size, allow_single_cluster=False):
    """(labels int32[n], probabilities float64[n]) of the model."""
    if n == 1:
        return np.full(1, -1, np.int32), np.zeros(1)
    merges = single_linkage(n, a, b, w)
    entries, clusters = condense(n, merges, min_cluster_size)
    return labels_from_condensed(n, entries, clusters, allow_single_cluster)
