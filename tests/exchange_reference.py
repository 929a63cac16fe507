"""A plain model of the exchange owner's path (graph.hip: merge_bounds_kernel,
merge_rank_kernel, group_count_kernel / group_sum_kernel, split_kernel,
split_kc_kernel, diag_totals_kernel, edges_count_kernel, edges_write_kernel)
and inputs that sit on those kernels' limits.  No device calls here:
tests/test_exchange_reference_cpu.py checks the model against a brute-force
dict and the CPU ops of tests/test_distributed_cpu.py, and every builder
against its own condition; tests/test_gpu_owner_merge.py runs the inputs.

The model is written from the definition: merged list = sorted unique keys
a << 32 | b with the counts of equal keys summed; split = first key with
a >= bound; totals = the summed counts of the diagonal keys; an edge is a key
whose summed count is not 0 (the diagonal is one only in KARMA_MODE_EQ), with
weight ((s / tA) + (s / tB)) / 2, one IEEE binary64 operation each on
int64 -> f64 conversions, and 0.0 with a zero-division flag where a total is 0.

What the builders restate of the device code, so that an input lands where it
is meant to:
  * the windows of merge_bounds_kernel and the greedy LDS staging of
    merge_rank_kernel                       -> windows()
  * the host loop of karma_pairs_merge_runs -> merge_launches()
The constants come from the library (karma_merge_tile) when it is built, so a
retuned tile moves the cases with it.
"""
import functools
import os
import types

import numpy as np

from karma_amd import _lib

TILE, LDS, MAX_RUNS, MG = _lib.merge_tile() if os.path.exists(_lib.LIB_PATH) else (1024, 6144, 64, 16)
ET = 1024            # elements per block of the edge stage and the group sums (kET)
READS, EQ = 0, 1     # KARMA_MODE_READS, KARMA_MODE_EQ
U64 = np.uint64


# ---- the model ----------------------------------------------------------------------
def key(a, b):
    return (np.asarray(a, U64) << U64(32)) | np.asarray(b, U64)


def ab(keys):
    keys = np.asarray(keys, U64)
    return (keys >> U64(32)).astype(np.int64), (keys & U64(0xFFFFFFFF)).astype(np.int64)


def merge(keys, counts, runs=None):
    """Sorted unique keys with the counts of equal keys summed."""
    keys, counts = np.asarray(keys, U64), np.asarray(counts, np.int64)
    assert runs is None or sum(runs) == len(keys)
    u, inv = np.unique(keys, return_inverse=True)
    c = np.zeros(len(u), np.int64)
    np.add.at(c, inv.reshape(-1), counts)
    return u, c


def split(keys, bounds):
    """Index of the first key with a >= bounds[r]."""
    return np.searchsorted(np.asarray(keys, U64), np.asarray(bounds, U64) << U64(32)).astype(np.int64)


def totals(keys, counts, N):
    a, b = ab(keys)
    t = np.zeros(N, np.int64)
    d = a == b
    np.add.at(t, a[d], np.asarray(counts, np.int64)[d])
    return t


diag_totals = totals  # edges() has an argument of that name


def edges(keys, counts, N, mode, totals=None):
    u, c = merge(keys, counts)
    tot = diag_totals(u, c, N) if totals is None else np.asarray(totals, np.int64).copy()
    a, b = ab(u)
    assert not len(u) or max(a.max(), b.max()) < N, "a contig id >= N breaks the entry points' contract"
    keep = c != 0
    if mode == READS:
        keep &= a != b
        assert totals is not None or np.all(a <= b), "a > b with list totals breaks the contract"
    a, b, s = a[keep], b[keep], c[keep]
    ta, tb = tot[a], tot[b]
    zero = (ta == 0) | (tb == 0)
    sf = s.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (sf / ta.astype(np.float64) + sf / tb.astype(np.float64)) / 2.0
    w[zero] = 0.0
    return types.SimpleNamespace(a=a.astype(np.uint32), b=b.astype(np.uint32), shared=s, weight=w, totals=tot,
                                 zero_div=bool(zero.any()))


def sorted_runs(keys, runs):
    off = np.r_[0, np.cumsum(runs)].astype(np.int64)
    runs_k = [keys[off[r]:off[r + 1]] for r in range(len(runs))]
    return all(bool(np.all(k[1:] >= k[:-1])) for k in runs_k)


def stable_merge(keys, counts, runs):
    """The unsummed merged list: by key, equal keys in run order (merge_rank_kernel's output)."""
    o = np.argsort(np.asarray(keys, U64), kind="stable")
    return np.asarray(keys, U64)[o], np.asarray(counts, np.int64)[o]


# ---- the merge kernels' window arithmetic -------------------------------------------
def windows(keys, runs):
    """One entry per block of merge_rank_kernel (a tile of one run), for at most
    MAX_RUNS sorted runs: lens[s] = whi - wlo of run s (counts of the tile's
    first and last key: <= for runs before, < for runs after), and the greedy
    staging: a window is staged while used + len <= LDS, else searched in
    place without advancing used."""
    keys = np.asarray(keys, U64)
    nr = len(runs)
    assert nr <= MAX_RUNS
    off = np.r_[0, np.cumsum(runs)].astype(np.int64)
    blocks = []
    for r in range(nr):
        n_t = -(-int(runs[r]) // TILE)
        if not n_t:
            continue
        t0 = off[r] + TILE * np.arange(n_t, dtype=np.int64)
        t1 = np.minimum(off[r + 1], t0 + TILE)
        k0, k1 = keys[t0], keys[t1 - 1]
        lens = np.zeros((n_t, nr), np.int64)
        for s in range(nr):
            if s == r:
                continue
            run = keys[off[s]:off[s + 1]]
            side = "right" if s < r else "left"
            lo = np.searchsorted(run, k0, side)
            lens[:, s] = np.maximum(lo, np.searchsorted(run, k1, side)) - lo
        for t in range(n_t):
            used, staged, inplace = 0, [], []
            for s in range(nr):
                if s == r:
                    continue
                ln = int(lens[t, s])
                if used + ln <= LDS:
                    staged.append(s)
                    used += ln
                else:
                    inplace.append(s)
            blocks.append(types.SimpleNamespace(run=r, tile=t, lens=lens[t].tolist(), staged=staged,
                                                inplace=inplace, used=used))
    return blocks


def rank_counts(keys, runs, r, s):
    """What the elements of run r count of run s (the answers of count_before)."""
    off = np.r_[0, np.cumsum(runs)].astype(np.int64)
    return np.searchsorted(keys[off[s]:off[s + 1]], keys[off[r]:off[r + 1]], "right" if s < r else "left")


def merge_launches(runs, kc=False, lazy=False):
    """{kernel: launches} of one karma_pairs_merge_runs{,_kc} call, as its host
    loop computes them (lazy: device input of at most MAX_RUNS runs, which
    leaves the group sums to the first accessor)."""
    runs = [int(x) for x in runs]
    n, nr = sum(runs), len(runs)
    out = {"merge_bounds": 0, "merge_rank": 0, "merge_split": 0, "merge_groups": 0, "merge_sum": 0}
    if nr <= MAX_RUNS:
        pairs = 1 if any(runs) else 0
        summed = not lazy
    else:
        o, pairs, summed = np.r_[0, np.cumsum(runs)].tolist(), 0, True
        out["merge_split"] = 1 if kc and n else 0
        while len(o) > 2:
            nxt = [0]
            for g0 in range(0, len(o) - 1, MAX_RUNS):
                g1 = min(len(o) - 1, g0 + MAX_RUNS)
                nxt.append(o[g1])
                pairs += 1 if o[g1] > o[g0] and g1 - g0 > 1 else 0
            o = nxt
    out["merge_bounds"] = out["merge_rank"] = pairs
    out["merge_groups"] = out["merge_sum"] = 1 if summed and n else 0
    return out


def merge_levels(n_runs):
    lv = 0
    while n_runs > 1:
        n_runs = -(-n_runs // MAX_RUNS)
        lv += 1
    return lv


# ---- case builders ------------------------------------------------------------------
# A case: keys, counts (all runs, concatenated), runs (lengths), N (contigs),
# sorted (False: KARMA_ERR_UNSORTED is due).  Every id is < N and a <= b.
A0 = 1000  # the first contig of the index keys: a merged slice does not start at contig 0


def G(i):
    """Index -> key, increasing: contig A0 + i // 2 with its diagonal (even i) and
    the pair with the next contig (odd i).  A list of the indices [0, U), U
    odd, holds the diagonal of every endpoint."""
    i = np.asarray(i, np.int64)
    a = A0 + i // 2
    return key(a, a + i % 2)


def G_N(U):
    return A0 + (U - 1) // 2 + 2


def counts_for(rng, n, hi=1 << 40):
    return rng.integers(1, hi, n, dtype=np.int64)


def mk(keys, counts, runs, N, sorted_=True, **kw):
    keys, counts = np.ascontiguousarray(keys, U64), np.ascontiguousarray(counts, np.int64)
    runs = [int(x) for x in runs]
    assert sum(runs) == len(keys) == len(counts)
    assert sorted_runs(keys, runs) == sorted_, "the case's runs are not in the order its name says"
    a, b = ab(keys)
    assert not len(keys) or (max(a.max(), b.max()) < N and np.all(a <= b))
    keys.setflags(write=False)
    counts.setflags(write=False)
    return types.SimpleNamespace(keys=keys, counts=counts, runs=runs, N=int(N), sorted=sorted_, **kw)


def subsets(rng, U, lens):
    """Runs that are sorted random subsets of the indices [0, U)."""
    return np.concatenate([np.sort(rng.choice(U, ln, replace=False)) for ln in lens] or [np.zeros(0, np.int64)])


@functools.lru_cache(maxsize=None)
def build_tile_lengths():
    rng = np.random.default_rng(101)
    lens = [1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]
    U = 3 * TILE + 1
    idx = subsets(rng, U, lens)
    c = mk(G(idx), counts_for(rng, len(idx)), lens, G_N(U))
    tiles = {}
    for bl in windows(c.keys, c.runs):
        tiles[bl.run] = tiles.get(bl.run, 0) + 1
    assert [tiles[r] for r in range(6)] == [1, 1, 1, 2, 2, 3]
    assert len(np.unique(c.keys)) < len(c.keys)  # keys shared between runs
    return c


@functools.lru_cache(maxsize=None)
def build_empty_runs(lens):
    rng = np.random.default_rng(102)
    U = 2 * max(max(lens), 1000) + 1
    idx = subsets(rng, U, lens)
    return mk(G(idx), counts_for(rng, len(idx)), lens, G_N(U))


@functools.lru_cache(maxsize=None)
def build_ties(W, L=None):
    """W runs that all hold the same L keys: the list is one run's, every count the sum over the runs."""
    L = TILE + 1 if L is None else L
    rng = np.random.default_rng(103 + W)
    keys = np.tile(G(np.arange(L)), W)
    c = mk(keys, counts_for(rng, W * L), [L] * W, G_N(L))
    u, s = merge(c.keys, c.counts)
    assert len(u) == L and np.array_equal(s, c.counts.reshape(W, L).sum(0))
    return c


@functools.lru_cache(maxsize=None)
def build_repeat_in_run():
    """A key repeated inside one run (twice, and one key five times across the
    tile edge) and also present in the others."""
    rng = np.random.default_rng(110)
    L = TILE + 301
    one = np.arange(L)
    rep = np.sort(np.r_[one, one[::3]])
    rep = np.sort(np.r_[rep, [rep[TILE - 1]] * 3])
    assert rep[TILE - 2] < rep[TILE - 1] == rep[TILE] == rep[TILE + 2]
    idx = np.r_[one, rep, one[1::2]]
    return mk(G(idx), counts_for(rng, len(idx)), [L, len(rep), len(one[1::2])], G_N(L))


@functools.lru_cache(maxsize=None)
def build_all_identical(W=64):
    """W runs x (TILE + 1) of one key (a diagonal): one group, summed by one thread."""
    rng = np.random.default_rng(111)
    L = TILE + 1
    keys = np.full(W * L, key(A0 + 3, A0 + 3), U64)
    c = mk(keys, counts_for(rng, W * L, 1 << 30), [L] * W, A0 + 10)
    assert all(bl.used == 0 for bl in windows(c.keys, c.runs))  # every window is empty: all before, or none
    return c


BOUND_L = (1, MG - 1, MG, MG + 1, 2 * MG - 1, 2 * MG + 1, MG * MG - 1, MG * MG, MG * MG + 1, MG * (MG + 1),
           MG * (MG + 1) + 1, MG ** 3 + 1)


@functools.lru_cache(maxsize=None)
def build_bound_search(L, searched_first, dup=False):
    """A run of L distinct keys (contig, contig + 2), or of L copies of one key,
    searched by a run that holds each of its keys and each key -1 and +1
    (contig + 1, contig + 3): every count 0..L is an answer of the in-window
    search.  Around them, runs of one key each: their tiles' first and last key
    is that key, so the MG-way bound search over the L keys (a range of
    exactly L) answers it too: every count 0..L when L + 1 <= the runs left,
    else counts spread evenly with both ends.  searched_first: the searched
    run comes first (<=), else last (<)."""
    rng = np.random.default_rng(120 + L)
    ctg = A0 + 4 * np.arange(L, dtype=np.int64)
    other = key(ctg, ctg + 2) if not dup else np.full(L, key(A0 + 40, A0 + 42), U64)
    base = np.unique(other)
    searching = np.unique(np.r_[base - U64(1), base, base + U64(1)])
    # single-key runs: answer c of the bound search for c in want
    n_probe = min(L + 1, MAX_RUNS - 2)
    want = np.unique(np.round(np.linspace(0, L, n_probe)).astype(np.int64))
    if dup:
        probes = np.r_[base - U64(1), base, base + U64(1)]
    elif searched_first:   # count of keys <= k is c: k = other[c - 1] (c >= 1), or below all
        probes = np.array([other[c - 1] if c else other[0] - U64(1) for c in want], U64)
    else:                  # count of keys < k is c: k = other[c] (c < L), or above all
        probes = np.array([other[c] if c < L else other[-1] + U64(1) for c in want], U64)
    runs_k = [searching] + [np.array([k], U64) for k in probes]
    runs_k = [other] + runs_k if searched_first else runs_k + [other]
    keys = np.concatenate(runs_k)
    lens = [len(x) for x in runs_k]
    N = int(ctg[-1]) + 8 if not dup else A0 + 50
    c = mk(keys, counts_for(rng, len(keys)), lens, N)
    s = 0 if searched_first else len(lens) - 1
    r = 1 if searched_first else 0
    ans = rank_counts(c.keys, c.runs, r, s)
    got = set()
    for p in range(len(probes)):
        got |= set(rank_counts(c.keys, c.runs, (2 if searched_first else 1) + p, s).tolist())
    if dup:
        assert set(ans.tolist()) == {0, L} and got == {0, L}
    else:
        assert set(ans.tolist()) == set(range(L + 1))
        assert got == set(want.tolist()) and {0, L} <= got and (L + 1 > n_probe or len(got) == L + 1)
    return c


@functools.lru_cache(maxsize=None)
def build_window(lens_in, tail=50):
    """Run 0 is one tile; run s >= 1 has exactly lens_in[s - 1] keys inside run
    0's key range [first, last) and `tail` past it.  Run 0 holds every 10th
    index, so the others tie with it."""
    rng = np.random.default_rng(130 + len(lens_in) + sum(lens_in))
    span = 10 * (TILE - 1)
    run0 = 10 * np.arange(TILE)
    parts = [run0]
    for j, ln in enumerate(lens_in):
        assert ln <= span
        inside = np.sort(rng.choice(span, ln, replace=False)) if j else np.arange(ln)
        parts.append(np.r_[inside, span + 1 + np.arange(tail)])
    idx = np.concatenate(parts)
    c = mk(G(idx), counts_for(rng, len(idx)), [len(x) for x in parts], G_N(span + tail + 2))
    bl = windows(c.keys, c.runs)[0]
    assert (bl.run, bl.tile) == (0, 0) and bl.lens[1:] == list(lens_in)
    used, staged = 0, []
    for s, ln in enumerate(lens_in, 1):
        if used + ln <= LDS:
            staged.append(s)
            used += ln
    assert bl.staged == staged and bl.used == used
    return c


def window_block0(name):
    c = case(name)
    return windows(c.keys, c.runs)[0]


@functools.lru_cache(maxsize=None)
def build_many_runs(W, mean, empty_group=None):
    """W > MAX_RUNS runs of random lengths around `mean`; every 7th run is empty,
    and the runs of the MAX_RUNS-group `empty_group` all are."""
    rng = np.random.default_rng(140 + W)
    lens = rng.integers(0, 2 * mean + 1, W)
    lens[3::7] = 0
    if empty_group is not None:
        lens[empty_group * MAX_RUNS:(empty_group + 1) * MAX_RUNS] = 0
    if W % MAX_RUNS == 1:
        lens[-1] = max(lens[-1], 5)  # the lone run has something to carry
    U = 4 * int(lens.max()) + 1
    idx = subsets(rng, U, lens.tolist())
    c = mk(G(idx), counts_for(rng, len(idx)), lens.tolist(), G_N(U))
    assert W > MAX_RUNS and len(np.unique(c.keys)) < len(c.keys)
    return c


def descend(c, at):
    """Case c with the keys at positions at, at + 1 (distinct) swapped."""
    keys = c.keys.copy()
    assert keys[at] != keys[at + 1]
    keys[at], keys[at + 1] = c.keys[at + 1], c.keys[at]
    off = np.r_[0, np.cumsum(c.runs)]
    r = int(np.searchsorted(off, at, "right")) - 1
    inside = at + 1 < off[r + 1]
    return mk(keys, c.counts, c.runs, c.N, sorted_=not inside)


@functools.lru_cache(maxsize=None)
def build_order(kind):
    rng = np.random.default_rng(150)
    lens = [300, 2 * TILE + 5, 700]
    idx = np.concatenate([np.sort(rng.choice(6001, ln, replace=False)) for ln in lens])
    base = mk(G(idx), counts_for(rng, len(idx)), lens, G_N(6001))
    off = np.r_[0, np.cumsum(lens)]
    if kind == "tile_edge":        # elements TILE - 1 | TILE of run 1
        return descend(base, int(off[1]) + TILE - 1)
    if kind == "run_end":          # the last two elements of run 1
        return descend(base, int(off[2]) - 2)
    if kind == "last_run":
        return descend(base, int(off[3]) - 2)
    if kind == "first_pair":       # the first two elements of run 0
        return descend(base, 0)
    if kind == "run_boundary":     # the last key of run 0 is above the first of run 1: no error
        assert base.keys[off[1] - 1] > base.keys[off[1]]
        return base
    if kind == "equal_adjacent":   # equal adjacent keys in a run: no error
        idx2 = idx.copy()
        idx2[off[1] + TILE] = idx2[off[1] + TILE - 1]
        idx2[off[3] - 1] = idx2[off[3] - 2]
        return mk(G(idx2), base.counts, lens, base.N)
    if kind in ("many_runs", "many_runs_lone"):  # a descent inside a run of a 65-run input (and inside the lone run)
        c = build_many_runs(65, 40)
        o = np.r_[0, np.cumsum(c.runs)]
        r = 64 if kind == "many_runs_lone" else int(np.argmax(np.array(c.runs[:64])))
        assert c.runs[r] >= 3
        return descend(c, int(o[r + 1]) - 2)
    raise KeyError(kind)


def to_runs(mk_keys, mk_counts, W, rng):
    """A merged (sorted, equal keys adjacent) list dealt out to W runs: the j-th
    of equal keys goes to run j, a single key to a random run.  The stable
    merge of the runs is the list again."""
    mk_keys = np.asarray(mk_keys, U64)
    n = len(mk_keys)
    head = np.r_[True, mk_keys[1:] != mk_keys[:-1]] if n else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(head, np.arange(n), 0)) if n else np.zeros(0, np.int64)
    occ = np.arange(n) - start
    single = head & np.r_[head[1:], True] if n else head
    run = np.where(single, rng.integers(0, W, n), occ)
    assert not n or run.max() < W
    o = np.argsort(run, kind="stable")
    lens = np.bincount(run, minlength=W).tolist()
    keys, counts = mk_keys[o], np.asarray(mk_counts, np.int64)[o]
    k2, c2 = stable_merge(keys, counts, lens)
    assert np.array_equal(k2, mk_keys) and np.array_equal(c2, mk_counts)
    return keys, counts, lens


def with_dups(keys, counts, rng, share=0.3, W=3):
    """A unique list with some keys made groups of 2..W elements whose counts
    add up to the key's; a key of count 0 becomes a group of nonzero counts
    (-7 (r - 1), 7, ..., 7), so only its sum says that it is no edge."""
    n = len(keys)
    rep = np.where(rng.random(n) < share, rng.integers(2, W + 1, n), 1)
    first = np.r_[0, np.cumsum(rep)[:-1]].astype(np.int64)
    part = np.where(counts == 0, 7, counts // (W + 1))
    k, c = np.repeat(keys, rep), np.repeat(part, rep)
    c[first] = counts - part * (rep - 1)
    assert np.array_equal(merge(k, c)[1], counts)
    return k, c


@functools.lru_cache(maxsize=None)
def build_totals_fill(n_past, zero_div):
    """The list of an owner whose contigs leave gaps: the count kernel fills
    totals that no key of the list names.  First contig 7; 0, 1, 2 and 1,500
    absent contigs between consecutive a; contig `bare` has no diagonal (its
    first key is a pair of count 0, which is no edge); N = last + n_past.
    zero_div: another bare contig has a real edge."""
    rng = np.random.default_rng(160 + n_past)
    step = [1, 2, 3, 1, 1501, 1, 2, 1501, 3, 1, 1, 2]
    ctg = 7 + np.cumsum(np.r_[0, np.tile(step, 4)])
    bare, bare_edge = int(ctg[9]), int(ctg[20])
    rows = []  # (a, b, count)
    for p, a in enumerate(ctg.tolist()):
        if a == bare:
            rows.append((a, int(ctg[p + 1]), 0))
        elif a == bare_edge and zero_div:
            rows.append((a, int(ctg[p + 2]), 5))
        else:
            rows.append((a, a, int(rng.integers(50, 1 << 20))))
            rows += [(a, int(ctg[q]), int(rng.integers(1, 50))) for q in (p + 1, p + 3)
                     if q < len(ctg) and int(ctg[q]) not in (bare, bare_edge)]
    ka, kb, kc = (np.array(x, np.int64) for x in zip(*rows))
    u = key(ka, kb)
    assert np.all(u[1:] > u[:-1])
    N = int(ctg[-1]) + n_past
    k, c = with_dups(u, kc, rng)
    keys, counts, lens = to_runs(k, c, 3, rng)
    case_ = mk(keys, counts, lens, N)
    m = edges(case_.keys, case_.counts, N, READS)
    a = np.unique(ab(u)[0])
    assert a[0] > 0 and {1, 2, 3, 1501} <= set(np.diff(a).tolist()) and m.zero_div == zero_div
    assert m.totals[bare] == 0 and (m.totals == 0).sum() > 3000 and N - 1 - a[-1] == n_past - 1
    return case_


@functools.lru_cache(maxsize=None)
def build_slice(zero_div):
    """An owner's slice: every a in [40,000, 41,000) of N = 100,000 contigs.
    zero_div: some b lie in other owners' slices, whose totals the owner has
    not gathered yet."""
    rng = np.random.default_rng(170)
    lo, hi, N = 40_000, 41_000, 100_000
    a = np.sort(rng.choice(np.arange(lo, hi), 700, replace=False))
    ka, kb = [a], [a]
    for d in (1, 5):
        ka.append(a[:-d]); kb.append(a[d:])
    if zero_div:
        ka.append(a[::9]); kb.append(rng.integers(hi, N, len(a[::9])))
    u = np.unique(key(np.concatenate(ka), np.concatenate(kb)))
    k, c = with_dups(u, counts_for(rng, len(u), 1 << 30), rng)
    keys, counts, lens = to_runs(k, c, 3, rng)
    case_ = mk(keys, counts, lens, N)
    m = edges(case_.keys, case_.counts, N, READS)
    assert m.zero_div == zero_div and np.count_nonzero(m.totals) == 700
    return case_


@functools.lru_cache(maxsize=None)
def build_edge_blocks(kind):
    """Lists on the edge stage's block edges (ET elements per block)."""
    rng = np.random.default_rng(180)
    if kind.startswith("n_"):      # a unique list of exactly n keys in two runs: n is the same summed or not
        n = ET + int(kind[2:])
        assert n % 2 == 1 or n == ET
        u = G(np.arange(n if n % 2 else n + 1))
        if n % 2 == 0:
            u = np.delete(u, 1)    # drop one pair, keep every diagonal
        k, c = u, counts_for(rng, n)
        W = 2
    elif kind == "group_across":   # elements ET - 2 .. ET + 1 of the unsummed list are one key
        u = G(np.arange(3 * ET - 1))
        rep = np.ones(len(u), np.int64)
        rep[ET - 2] = 4
        k = np.repeat(u, rep)
        c = counts_for(rng, len(k))
        assert k[ET - 2] == k[ET + 1] != k[ET + 2] and k[ET - 3] != k[ET - 2]
        W = 4
    elif kind == "empty_block":    # block 1 (elements ET .. 2 ET - 1) holds no edge, blocks 0 and 2 do
        a0 = A0 + np.arange(ET // 2)
        d = A0 + ET // 2 + np.arange(ET)            # diagonals only, or pairs of count 0
        a2 = d[-1] + 1 + np.arange(ET // 2)
        u = np.r_[key(np.repeat(a0, 2), np.repeat(a0, 2) + np.tile([0, 1], len(a0))), key(d, d),
                  key(np.repeat(a2, 2), np.minimum(np.repeat(a2, 2) + np.tile([0, 1], len(a2)), a2[-1]))]
        u = np.unique(u)
        k, c = u, counts_for(rng, len(u))
        c[ET + 5] = 0              # a diagonal of count 0: its contig's total is 0, nobody points at it
        m = edges(k, c, int(a2[-1]) + 1, READS)
        blk = np.searchsorted(k, key(m.a, m.b)) // ET
        assert set(blk.tolist()) == {0, 2} and len(k) > 2 * ET
        W = 2
    elif kind == "diagonals_only":
        d = A0 + 3 * np.arange(ET + 77)
        k, c = key(d, d), counts_for(rng, len(d))
        W = 2
    else:
        raise KeyError(kind)
    keys, counts, lens = to_runs(k, c, W, rng)
    a, b = ab(k)
    return mk(keys, counts, lens, int(max(a.max(), b.max())) + 1)


def recip_differs(s, t):
    s, t = s.astype(np.float64), t.astype(np.float64)
    return s / t != s * (1.0 / t)


@functools.lru_cache(maxsize=None)
def build_weights():
    """Counts and totals up to 2^40, and some above 2^53 with odd low bits (the
    int64 -> f64 conversion rounds); at least 100 of the divisions differ
    from a multiplication by the reciprocal; pairs of count 0 are no edges."""
    for seed in range(190, 200):
        rng = np.random.default_rng(seed)
        T = 600
        ctg = A0 + np.arange(T)
        tot = rng.integers(1, 1 << 40, T, dtype=np.int64)
        tot[::7] = (rng.integers(1 << 53, 1 << 60, len(tot[::7]), dtype=np.int64)) | 1
        ka, kb, kc = [ctg], [ctg], [tot]
        for d in (1, 2, 5):
            s = rng.integers(1, 1 << 40, T - d, dtype=np.int64)
            s[::5] = (rng.integers(1 << 53, 1 << 59, len(s[::5]), dtype=np.int64)) | 1
            s[3::11] = 0
            ka.append(ctg[:-d]); kb.append(ctg[d:]); kc.append(s)
        u, o = np.unique(key(np.concatenate(ka), np.concatenate(kb)), return_index=True)
        cnt = np.concatenate(kc)[o]
        k, c = with_dups(u, cnt, rng)
        keys, counts, lens = to_runs(k, c, 3, rng)
        case_ = mk(keys, counts, lens, A0 + T)
        m = edges(case_.keys, case_.counts, case_.N, READS)
        differ = int(recip_differs(m.shared, m.totals[m.a]).sum() + recip_differs(m.shared, m.totals[m.b]).sum())
        if differ >= 100 and not m.zero_div:
            assert (cnt == 0).sum() > 50 and len(m.a) == (cnt != 0).sum() - T
            assert (m.shared > 1 << 53).sum() > 50 and (m.shared & 1)[m.shared > 1 << 53].all()
            case_.recip_differ = differ
            return case_
    raise AssertionError("no seed gives 100 divisions that differ from reciprocal multiplication")


# every case of the GPU tests: name -> (builder, args)
CASES = {
    "tile_lengths": (build_tile_lengths, ()),
    "empty_first_middle_last": (build_empty_runs, ((0, 700, 0, TILE + 300, 0),)),
    "one_run": (build_empty_runs, ((2 * TILE + 500,),)),
    "one_key": (build_empty_runs, ((1,),)),
    "all_empty": (build_empty_runs, ((0, 0, 0, 0),)),
    "ties_2": (build_ties, (2,)),
    "ties_3": (build_ties, (3,)),
    "ties_63": (build_ties, (MAX_RUNS - 1,)),
    "ties_64": (build_ties, (MAX_RUNS,)),
    "repeat_in_run": (build_repeat_in_run, ()),
    "all_identical": (build_all_identical, ()),
    "window_6143": (build_window, ((LDS - 1,),)),
    "window_6144": (build_window, ((LDS,),)),
    "window_6145": (build_window, ((LDS + 1,),)),
    "window_3072_3072": (build_window, ((LDS // 2, LDS // 2),)),
    "window_3072_3073": (build_window, ((LDS // 2, LDS // 2 + 1),)),
    "window_spill_then_small": (build_window, ((LDS + 1, 10),)),
    "window_spill_between": (build_window, ((4000, 3000, LDS - 4000),)),
    "runs_65": (build_many_runs, (MAX_RUNS + 1, 40)),
    "runs_129": (build_many_runs, (2 * MAX_RUNS + 1, 30, 1)),
    "runs_4097": (build_many_runs, (MAX_RUNS * MAX_RUNS + 1, 6, 2)),
    "order_ok_run_boundary": (build_order, ("run_boundary",)),
    "order_ok_equal_adjacent": (build_order, ("equal_adjacent",)),
    "totals_last_plus_1": (build_totals_fill, (1, False)),
    "totals_last_plus_2": (build_totals_fill, (2, False)),
    "totals_last_plus_5000": (build_totals_fill, (5000, False)),
    "totals_last_plus_1_zero_div": (build_totals_fill, (1, True)),
    "totals_last_plus_2_zero_div": (build_totals_fill, (2, True)),
    "totals_last_plus_5000_zero_div": (build_totals_fill, (5000, True)),
    "slice": (build_slice, (False,)),
    "slice_zero_div": (build_slice, (True,)),
    "edges_n_1023": (build_edge_blocks, ("n_-1",)),
    "edges_n_1024": (build_edge_blocks, ("n_0",)),
    "edges_n_1025": (build_edge_blocks, ("n_1",)),
    "edges_group_across_blocks": (build_edge_blocks, ("group_across",)),
    "edges_empty_block": (build_edge_blocks, ("empty_block",)),
    "edges_diagonals_only": (build_edge_blocks, ("diagonals_only",)),
    "weights": (build_weights, ()),
}
for _L in BOUND_L:
    CASES[f"bound_{_L}_le"] = (build_bound_search, (_L, True))
    CASES[f"bound_{_L}_lt"] = (build_bound_search, (_L, False))
CASES["bound_dup_le"] = (build_bound_search, (2 * MG + 1, True, True))
CASES["bound_dup_lt"] = (build_bound_search, (2 * MG + 1, False, True))

# inputs with a descent inside a run: KARMA_ERR_UNSORTED
UNSORTED = {
    "tile_edge": (build_order, ("tile_edge",)),
    "run_end": (build_order, ("run_end",)),
    "last_run": (build_order, ("last_run",)),
    "first_pair": (build_order, ("first_pair",)),
    "many_runs": (build_order, ("many_runs",)),
    "many_runs_lone": (build_order, ("many_runs_lone",)),
}

# the cases whose totals the count kernel has to fill past the list's own contigs
TOTALS_FILL = tuple(k for k in CASES if k.startswith(("totals_", "slice")))


def case(name):
    builder, args = (CASES.get(name) or UNSORTED[name])
    return builder(*args)


@functools.lru_cache(maxsize=None)
def case_model(name):
    """(merged keys, summed counts) of a case."""
    c = case(name)
    return merge(c.keys, c.counts, c.runs)


@functools.lru_cache(maxsize=None)
def case_edges(name, mode=READS, caller_totals=False):
    """The model's edges of a case; caller_totals: totals 1000 + 3 c for every contig c."""
    c = case(name)
    t = 1000 + 3 * np.arange(c.N, dtype=np.int64) if caller_totals else None
    return edges(c.keys, c.counts, c.N, mode, t)
