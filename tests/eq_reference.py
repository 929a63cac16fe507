"""Plain Python model of the eq-class graph (no test in here) and builders of
class lists that sit on the kernel boundaries of karma_amd/csrc/eq.hip and of
the eq half of graph.hip.  eq_model restates read_graph.py:86-131 with Python
ints, itertools.combinations and one dict; tests/test_eq_reference_cpu.py pins
oracle.graph_groups(..., dedup=False) to it, and tests/test_gpu_eq_graph.py
compares the device with the oracle on the fixtures built here.

A class list is (off int64[C + 1], mem uint32, cnt int64[C], skip uint8[C]):
class c holds mem[off[c]:off[c + 1]], its count and its size-token-"1" flag.
"""
import itertools

import numpy as np

K_SEG = 1024      # eq.hip kSeg: target entries of one seg_reduce run
K_SEG_CAP = 2048  # eq.hip kSegCap: LDS capacity of a run; longer runs merge-sort


def eq_model(off, mem, cnt, skip, n):
    """read_graph.py:86-131 on id arrays.  Returns a dict shaped like
    oracle.graph_groups: a, b, shared, first, weight sorted by (a, b), totals
    and zero_div (a kept pair over a zero total; its weight is left 0.0)."""
    off = [int(x) for x in off]
    mem = [int(x) for x in mem]
    cnt = [int(x) for x in cnt]
    flagged = skip is not None and len(skip) > 0
    totals = [0] * n
    pairs = {}  # (min, max) -> [sum, first emission index]
    t = 0
    for c in range(len(off) - 1):
        ids = mem[off[c]:off[c + 1]]
        for x in ids:
            totals[x] += cnt[c]
        if flagged and skip[c]:
            continue
        for x, y in itertools.combinations(ids, 2):
            e = pairs.setdefault((min(x, y), max(x, y)), [0, t])
            e[0] += cnt[c]
            t += 1
    assert all(abs(x) < 2 ** 53 for x in totals)
    a, b, s, f, w = [], [], [], [], []
    zero_div = False
    for (x, y), (sm, first) in sorted(pairs.items()):
        assert abs(sm) < 2 ** 53
        if sm == 0:
            continue
        if totals[x] == 0 or totals[y] == 0:
            zero_div, wt = True, 0.0
        else:
            wt = ((sm / totals[x]) + (sm / totals[y])) / 2
        a.append(x), b.append(y), s.append(sm), f.append(first), w.append(wt)
    every = sorted(pairs.items())  # the pair list: keys that sum to 0 included
    return dict(a=np.array(a, np.uint32), b=np.array(b, np.uint32), shared=np.array(s, np.int64),
                first=np.array(f, np.uint64), weight=np.array(w, np.float64), totals=np.array(totals, np.int64),
                zero_div=zero_div,
                pairs=(np.array([(x << 32) | y for (x, y), _ in every], np.uint64),
                       np.array([v[0] for _, v in every], np.int64), np.array([v[1] for _, v in every], np.uint64)))


def pair_lower_ids(off, mem, skip):
    """The lower contig of every emitted pair (any order), vectorised per class size."""
    off = np.asarray(off, np.int64)
    mem = np.asarray(mem, np.int64)
    m = np.diff(off)
    live = m >= 2
    if skip is not None and len(skip):
        live &= np.asarray(skip) == 0
    out = []
    for size in np.unique(m[live]).tolist():
        rows = off[:-1][live & (m == size)]
        block = mem[rows[:, None] + np.arange(size)[None, :]]
        i, j = np.triu_indices(size, 1)
        out.append(np.minimum(block[:, i], block[:, j]).ravel())
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def pair_list(off, mem, cnt, skip):
    """The pair list before the edge stage: every distinct key (a << 32 | b), its
    summed count (keys that sum to 0 included) and first emission index, sorted
    by key.  Vectorised per class size; int64 sums are exact."""
    off = np.asarray(off, np.int64)
    mem = np.asarray(mem, np.int64)
    cnt = np.asarray(cnt, np.int64)
    m = np.diff(off)
    p = m * (m - 1) // 2
    if skip is not None and len(skip):
        p = np.where(np.asarray(skip) != 0, 0, p)
    poff = np.zeros(len(m) + 1, np.int64)
    np.cumsum(p, out=poff[1:])
    keys, vals, idx = [], [], []
    for size in np.unique(m[p > 0]).tolist():
        sel = np.flatnonzero((p > 0) & (m == size))
        block = mem[off[sel][:, None] + np.arange(size)[None, :]]
        i, j = np.triu_indices(size, 1)  # combinations order
        x, y = block[:, i], block[:, j]
        keys.append(((np.minimum(x, y) << 32) | np.maximum(x, y)).ravel())
        vals.append(np.repeat(cnt[sel], len(i)))
        idx.append((poff[sel][:, None] + np.arange(len(i))[None, :]).ravel())
    if not keys:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint64)
    keys, vals, idx = np.concatenate(keys), np.concatenate(vals), np.concatenate(idx)
    uk, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uk), np.int64)
    np.add.at(sums, inv, vals)
    first = np.full(len(uk), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, inv, idx)
    return uk.astype(np.uint64), sums, first.astype(np.uint64)


def n_pairs(off, skip):
    m = np.diff(np.asarray(off, np.int64))
    p = m * (m - 1) // 2
    if skip is not None and len(skip):
        p = p[np.asarray(skip) == 0]
    return int(p.sum())


def run_lengths(off, mem, skip, n, cap=None):
    """Lengths of seg_reduce's runs (the rule at eq.hip "4. sort + reduce of
    whole segments"): the pairs are grouped by lower contig a, segoff[a] = pairs
    with a lower contig below a; run r is [lo(r), lo(r + 1)), lo(r) = P when
    r * kSeg >= P, else segoff of the first a with segoff[a] >= r * kSeg.
    There are ceil(max(cap, 1) / kSeg) runs; cap = the scratch capacity (the
    pair total P itself unless the call ran on a speculative capacity >= P)."""
    lower = pair_lower_ids(off, mem, skip)
    P = len(lower)
    cap = P if cap is None else cap
    assert cap >= P
    segoff = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(lower, minlength=n), out=segoff[1:])
    n_runs = -(-max(cap, 1) // K_SEG)
    lo = []
    for r in range(n_runs + 1):
        target = r * K_SEG
        lo.append(P if target >= P else int(segoff[np.searchsorted(segoff, target, side="left")]))
    return [lo[r + 1] - lo[r] for r in range(n_runs)]


# ---- builders ------------------------------------------------------------------------

def pack(classes):
    """[(members, count) or (members, count, skip)] -> (off, mem, cnt, skip)."""
    sizes = [len(c[0]) for c in classes]
    off = np.zeros(len(classes) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    mem = np.array([x for c in classes for x in c[0]], np.uint32)
    cnt = np.array([c[1] for c in classes], np.int64)
    skip = np.array([c[2] if len(c) > 2 else 0 for c in classes], np.uint8)
    return off, mem, cnt, skip


def anchors(ids, count=1_000_003):
    """One single-member class per contig (not skipped: totals, no pairs), so no
    total is zero whatever the pair counts add up to."""
    return [([int(x)], count) for x in ids]


def grouped_partners(L, first, sizes=(1, 2, 3, 4, 5)):
    """L partner ids from `first` up, in groups of equal ids whose sizes cycle
    through `sizes` (the last group cut to fit)."""
    out, v = [], first
    for g in itertools.cycle(sizes):
        if len(out) >= L:
            break
        out += [v] * min(g, L - len(out))
        v += 1
    return out


_COUNTS = (3, -2, 7, 1, -5, 4, 0, 2, -1, 6, 9)


def star(hub, partners, seed, counts=_COUNTS):
    """One two-member class per partner, holding `hub` (the lower id) and the
    partner in either order, with counts that include negatives and zero, in
    shuffled order: len(partners) pairs whose lower contig is `hub`."""
    rng = np.random.default_rng(seed)
    out = []
    for i, v in enumerate(partners):
        assert v >= hub
        out.append(([hub, v] if i % 3 else [v, hub], counts[i % len(counts)]))
    return [out[i] for i in rng.permutation(len(out))]


def hub_fixture(prefix, L, seed=0, hub_sizes=(1, 2, 3, 4, 5)):
    """A hub contig (id 1) with L pairs as the lower id behind one segment of
    `prefix` pairs on contig 0; partners repeat in groups of 1 to 5, counts
    include negatives.  Returns (classes, n)."""
    pp = grouped_partners(prefix, 2)
    hp = grouped_partners(L, 2, hub_sizes)
    n = max(pp + hp + [1]) + 1
    classes = star(0, pp, seed + 1) + star(1, hp, seed + 2)
    rng = np.random.default_rng(seed)
    classes = [classes[i] for i in rng.permutation(len(classes))]
    return classes + anchors(range(n)), n


def two_member_classes(P, n, seed):
    """Exactly P pairs from P two-member classes over n contigs, counts 1 to 8."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, n, (P, 2))
    off = np.arange(P + 1, dtype=np.int64) * 2
    return off, x.ravel().astype(np.uint32), rng.integers(1, 9, P).astype(np.int64), np.zeros(P, np.uint8)


def sized_classes(sizes, dup, n=400, seed=0, token1=()):
    """One class per entry of `sizes` with distinct members (dup: the last
    member of every class of >= 2 repeats its first, a self-pair) between small
    filler classes over the same contigs; positive counts.  Classes whose index
    in `sizes` is in `token1` carry the size token "1"."""
    rng = np.random.default_rng(seed)
    classes = []
    for i, m in enumerate(sizes):
        ids = rng.choice(n, m, replace=False).tolist()
        if dup and m >= 2:
            ids[-1] = ids[0]
        classes.append((rng.choice(n, 2, replace=False).tolist(), int(rng.integers(1, 9))))
        classes.append((ids, int(rng.integers(1, 9)), 1 if i in token1 else 0))
        classes.append((rng.choice(n, 3, replace=False).tolist(), int(rng.integers(1, 9))))
    return classes + anchors(range(n), 11), n


def straddle_fixture(pos, group, L, seed=0):
    """One hub (contig 0) with L pairs whose sorted run holds `group` equal keys
    at positions pos .. pos + group - 1 and single keys elsewhere; counts
    include negatives.  Returns (classes, n)."""
    partners = list(range(1, 1 + pos)) + [1 + pos] * group
    partners += list(range(2 + pos, 2 + pos + L - len(partners)))
    assert len(partners) == L
    n = max(partners) + 1
    return star(0, partners, seed, counts=(3, -2, 7, 1, -5, 4, 2, -1, 6, 9)) + anchors(range(n)), n


def sorted_run_keys(off, mem, skip, a):
    """The keys of the pairs whose lower contig is a, sorted (one segment)."""
    off = np.asarray(off, np.int64)
    keys = []
    for c in range(len(off) - 1):
        if skip is not None and len(skip) and skip[c]:
            continue
        for x, y in itertools.combinations([int(v) for v in mem[off[c]:off[c + 1]]], 2):
            if min(x, y) == a:
                keys.append(max(x, y))
    return sorted(keys)


def sparse_contigs(N, P=3000, active=24, seed=0):
    """P two-member classes over at most `active` contigs spread over [0, N):
    run targets fall among long stretches of tied segment offsets."""
    rng = np.random.default_rng(seed + N)
    ids = np.unique(np.linspace(0, N - 1, min(N, active)).astype(np.int64))
    x = ids[rng.integers(0, len(ids), (P, 2))]
    off = np.arange(P + 1, dtype=np.int64) * 2
    return off, x.ravel().astype(np.uint32), rng.integers(1, 9, P).astype(np.int64), np.zeros(P, np.uint8), N


def many_runs(P=80_000, n=4000, hub=0, seed=0):
    """P two-member classes over n contigs (segments of a few dozen pairs: one
    non-empty run per 1,024 pairs), and with hub > 0 a contig in the middle with
    `hub` more pairs as the lower id (its run is followed by empty ones)."""
    off, mem, cnt, skip = two_member_classes(P, n, seed)
    if hub:
        rng = np.random.default_rng(seed + 1)
        h = n // 2
        v = rng.integers(h + 1, n, hub)
        mem = np.concatenate([mem, np.stack([np.full(hub, h), v], 1).ravel().astype(np.uint32)])
        cnt = np.concatenate([cnt, rng.integers(-4, 9, hub)])
        off = np.arange(P + hub + 1, dtype=np.int64) * 2
        skip = np.zeros(P + hub, np.uint8)
    return off, mem, cnt, skip, n


def totals_fixture():
    """Empty classes at the start, in a row in the middle and at the end;
    single-member classes that are not skipped; counts of -2^31, negatives and
    zeros; totals that end negative (no kept pair meets a zero total)."""
    big = -2 ** 31
    classes = [([], 5), ([], -3),
               ([0, 1], 7), ([2], big), ([2, 3], 4), ([3], 9),
               ([], 1), ([], 0), ([], big),
               ([1, 4], 0), ([4], -6), ([0, 4, 5], -2), ([5], big), ([5, 0], 3), ([6], 0), ([1, 2], big),
               ([3, 3], -1), ([6, 6], 0),
               ([], 2), ([], 2)]
    return classes, 8


def scan_tiles(C, seed=0):
    """C two-member classes over n = C contigs, built vectorised: class c holds
    c and a random other contig, so every contig is a member."""
    rng = np.random.default_rng(seed)
    x = np.stack([np.arange(C), rng.integers(0, C, C)], 1)
    flip = rng.random(C) < 0.5
    x[flip] = x[flip][:, ::-1]
    off = np.arange(C + 1, dtype=np.int64) * 2
    return off, x.ravel().astype(np.uint32), rng.integers(1, 9, C).astype(np.int64), np.zeros(C, np.uint8), C


def edge_keys(K, width=7):
    """K distinct keys in sorted order: position i is (i // width, i // width + 1 + i % width)."""
    i = np.arange(K)
    a = i // width
    return a, a + 1 + i % width


def edge_fixture(K, zero_at=(), zero_total_at=None, seed=0):
    """A pair list of K distinct keys (edge_keys), each emitted once with a
    positive count, the keys at the sorted positions `zero_at` twice with +6
    and -6 (sum 0: kept in the pair list, dropped by the edge stage), classes
    shuffled.  zero_total_at: the higher contig of the kept key at that
    position gets a total of 0 (a single-member class takes its sum back), and
    every other key of that contig sums to 0, so that key alone meets it."""
    rng = np.random.default_rng(seed)
    a, b = edge_keys(K)
    n = int(b.max()) + 1
    zero = set(int(z) for z in zero_at)
    if zero_total_at is not None:
        z = int(b[zero_total_at])
        zero |= set(np.flatnonzero((a == z) | (b == z)).tolist()) - {zero_total_at}
    classes = []
    for i in range(K):
        pair = [int(a[i]), int(b[i])] if i % 2 else [int(b[i]), int(a[i])]
        if i in zero:
            classes += [(pair, 6), (pair[::-1], -6)]
        else:
            classes.append((pair, 1 + i % 9))
    classes = [classes[i] for i in rng.permutation(len(classes))]
    ids = list(range(n))
    if zero_total_at is not None:
        assert zero_total_at not in zero
        ids.remove(z)
        classes.append(([z], -sum(c[1] for c in classes for x in c[0] if x == z)))
    return classes + anchors(ids), n


def order_fixture(R, prefix, seed=0):
    """A run of R edges with the same lower contig and distinct partners, its
    classes emitted in shuffled order, behind `prefix` edges on lower contigs
    (runs of 10) and before 5 edges on higher ones.  Returns (classes, n, hub)."""
    rng = np.random.default_rng(seed + R)
    lows = -(-prefix // 10)
    hub = lows
    classes = [([i, hub + 1 + j], 2) for i in range(lows) for j in range(10)][:prefix]
    classes += [([hub, hub + 1 + j], 1 + j % 7) for j in range(R)]
    classes += [([hub + 1 + j, hub + 2 + j], 3) for j in range(5)]
    classes = [classes[i] for i in rng.permutation(len(classes))]
    return classes, hub + R + 7, hub


def short_runs(n_runs=300, seed=0):
    """Runs of 1, 2, 3, 1, ... edges per lower contig (a 256-edge block spans
    about 128 of them), classes shuffled.  Returns (classes, n)."""
    rng = np.random.default_rng(seed)
    classes = [([a, a + 1 + j], 1 + (a + j) % 5) for a in range(n_runs) for j in range(1 + a % 3)]
    classes = [classes[i] for i in rng.permutation(len(classes))]
    return classes, n_runs + 4
