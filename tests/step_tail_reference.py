"""A plain model of the deferred step's tail (step.hip: step_pack_kernel,
step_merge_kernel, step_edge_count_kernel, step_edge_write_kernel) and record
batches that sit on those kernels' limits.  No device calls here:
tests/test_step_tail_reference_cpu.py checks the model against the oracle and
a brute-force dict, and every builder against its own condition;
tests/test_gpu_step_tail.py runs the batches.

The tail is reachable only through karma_step_run, so an input is a batch of
records, not a list.  Every read here has one record (contig a) or two (a and
b, a < b <= a + 3): at most 8 records and a contig span <= 3, so every read
stays on the compact path, nothing votes for a relabel, and no bucket can
overflow (only general reads feed the hash).  A read {a} gives the key (a, a);
a read {a, b} gives (a, a), (a, b), (b, b); repeating a read raises the counts.

The model is written from the definition: a rank's list = the sorted unique
keys of its reads with their counts; owner r's runs = every rank's keys with
bounds[r] <= a < bounds[r + 1], in rank order; the graph = the edges of the
union of all ranks' reads (exchange_reference.edges).

What is restated of the device code, so that a batch lands where it is meant to:
  * run_offsets()  a bound's offset in a rank's list (0 below the range, U past
                   the last bucket, else the keys with a < bound)
  * windows()      per merge tile (MT elements of a run) its window in every
                   other run (<= for earlier runs, < for later ones), the greedy
                   LDS staging (a window that does not fit does not advance the
                   fill) and the fast path (all staged and at most MFAST runs)
  * slot_kc()      the slot size a synchronous sizing step leaves
The constants come from the library (karma_step_tail_tile) when it is built.
"""
import functools
import os
import types

import numpy as np

import exchange_reference as xr
import pairs_reference as pr
from karma_amd import _lib

K = _lib.step_tail_tile() if os.path.exists(_lib.LIB_PATH) else types.SimpleNamespace(
    MT=1024, MLDS=8192, MFAST=8, MG=16, ET=512, MAX_RUNS=64, merge_blocks=0, edge_blocks=0)
MT, MLDS, MFAST, ET, MAX_RUNS = K.MT, K.MLDS, K.MFAST, K.ET, K.MAX_RUNS
EDGE_BLOCKS = 4 * 256   # the edge stage's grid on a 256-CU device: the GPU test asserts it from the export
U64 = np.uint64
NS = types.SimpleNamespace


# ---- reads and records --------------------------------------------------------------
def reads(a, b=None, m=None):
    """Reads {a[i], b[i]} (b[i] == a[i]: one record), each m[i] times."""
    a = np.asarray(a, np.int64).reshape(-1)
    b = a.copy() if b is None else np.asarray(b, np.int64).reshape(-1)
    m = np.ones(len(a), np.int64) if m is None else np.broadcast_to(np.asarray(m, np.int64), a.shape).copy()
    assert len(a) == len(b) == len(m) and np.all(a <= b) and np.all(b - a <= 3) and np.all(m >= 1)
    assert not len(a) or a.min() >= 0
    return NS(a=a, b=b, m=m)


def cat(*rs):
    return NS(a=np.concatenate([r.a for r in rs]), b=np.concatenate([r.b for r in rs]),
              m=np.concatenate([r.m for r in rs]))


EMPTY = reads([])


def records(r, seed=0):
    """uint32[A, 2] (read id, contig): the reads in a seeded random order, ids
    rising, every other two-record read with its larger contig first."""
    a, b = np.repeat(r.a, r.m), np.repeat(r.b, r.m)
    o = np.random.default_rng(seed).permutation(len(a))
    a, b = a[o], b[o]
    two = b != a
    n = 1 + two.astype(np.int64)
    start = np.cumsum(n) - n
    rec = np.zeros((int(n.sum()), 2), np.uint32)
    rec[:, 0] = np.repeat(np.arange(len(a)), n)
    flip = two & (np.arange(len(a)) % 2 == 1)
    rec[start, 1] = np.where(flip, b, a)
    rec[start[two] + 1, 1] = np.where(flip, a, b)[two]
    return rec


def stays_deferred(rec, N):
    """From the model alone: no read of more than 8 records and no general read
    (a contig span > 3), hence no hash pair, no bucket overflow, no pair
    capacity and no relabel vote (pairs_reference.general_reads / relabels /
    hash_pairs_per_bucket say the same, read by read: the CPU tests compare)."""
    rec = np.asarray(rec, np.int64).reshape(-1, 2)
    if not len(rec):
        return True
    off = pr.read_bounds(rec)
    span = np.maximum.reduceat(rec[:, 1], off[:-1]) - np.minimum.reduceat(rec[:, 1], off[:-1])
    return pr.big_reads(rec) == 0 and int(span.max()) <= 3 and int(rec[:, 1].max()) < N


# ---- the model ----------------------------------------------------------------------
def pair_list(r):
    """(keys, counts) of one rank's reads: sorted unique a << 32 | b."""
    two = r.b != r.a
    k = np.concatenate([xr.key(r.a, r.a), xr.key(r.b, r.b)[two], xr.key(r.a, r.b)[two]])
    c = np.concatenate([r.m, r.m[two], r.m[two]])
    return xr.merge(k, c)


def graph(batches, N):
    """The edges and totals of the union of the ranks' reads."""
    ls = [pair_list(r) for r in batches]
    return xr.edges(np.concatenate([k for k, _ in ls]), np.concatenate([c for _, c in ls]), N, xr.READS)


def run_offsets(keys, bounds, N):
    """step_merge_kernel / step_pack_kernel: where owner bound bd starts in a rank's list."""
    g = pr.geometry(N)
    a = xr.ab(keys)[0]
    return np.array([0 if bd <= 0 else len(keys) if (int(bd) >> g.bw) >= g.B else int(np.searchsorted(a, bd))
                     for bd in bounds], np.int64)


def slices(batches, bounds, N):
    """lens[s][r]: keys rank s holds for owner r."""
    return [np.diff(run_offsets(pair_list(b)[0], bounds, N)).tolist() for b in batches]


def owner_runs(batches, bounds, N, r):
    """Owner r's merge input: (keys, counts, run lengths), the runs in rank order.
    One batch and several bounds: the emulated exchange (the rank's own slices)."""
    ks, cs, lens = [], [], []
    if len(batches) == 1 and len(bounds) > 2:
        k, c = pair_list(batches[0])
        o = run_offsets(k, bounds, N)
        return k, c, np.diff(o).tolist()
    for b in batches:
        k, c = pair_list(b)
        o = run_offsets(k, bounds, N)
        ks.append(k[o[r]:o[r + 1]])
        cs.append(c[o[r]:o[r + 1]])
        lens.append(int(o[r + 1] - o[r]))
    return np.concatenate(ks), np.concatenate(cs), lens


def windows(keys, runs):
    """One entry per tile of step_merge_kernel: run, tile, lens[s] (the window in
    run s), staged / inplace runs, used LDS keys, fast (the lockstep path)."""
    keys = np.asarray(keys, U64)
    nr = len(runs)
    assert nr <= MAX_RUNS
    off = np.r_[0, np.cumsum(runs)].astype(np.int64)
    out = []
    for r in range(nr):
        n_t = -(-int(runs[r]) // MT)
        if not n_t:
            continue
        t0 = off[r] + MT * np.arange(n_t, dtype=np.int64)
        t1 = np.minimum(off[r + 1], t0 + MT)
        k0, k1 = keys[t0], keys[t1 - 1]
        lens = np.zeros((n_t, nr), np.int64)
        for s in range(nr):
            if s == r or not runs[s]:
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
                if used + ln <= MLDS:
                    staged.append(s)
                    used += ln
                else:
                    inplace.append(s)
            out.append(NS(run=r, tile=t, lens=lens[t].tolist(), staged=staged, inplace=inplace, used=used,
                          fast=not inplace and nr <= MFAST))
    return out


def slot_kc(batches, bounds, N, kc=0):
    """The slot's key room after a synchronous step on these batches."""
    mx = max(max(s) for s in slices(batches, bounds, N))
    return max(kc, mx + mx // 4 + 1024)


def merged_unsummed(keys, counts, runs):
    return xr.stable_merge(keys, counts, runs)


# ---- batches -------------------------------------------------------------------------
def chain(ctg, pair=True, m1=1, m2=1):
    """Contigs ctg (ascending): a read {c} for each, and {c, next} where pair is
    set (the next contig at most 3 ids on).  Keys in list order: per contig its
    diagonal, then its pair."""
    ctg = np.asarray(ctg, np.int64)
    n = len(ctg)
    pair = np.broadcast_to(np.asarray(pair, bool), (n,)).copy()
    if n:
        pair[-1] = False
        pair[:-1] &= np.diff(ctg) <= 3
    m1 = np.broadcast_to(np.asarray(m1, np.int64), (n,))
    m2 = np.broadcast_to(np.asarray(m2, np.int64), (n,))
    nxt = np.r_[ctg[1:], 0] if n else ctg
    return cat(reads(ctg, None, m1), reads(ctg[pair], nxt[pair], m2[pair]))


def dirt(N, which, light=False):
    """A dirtying batch: every contig a nonzero total (9 or 14; light, for the
    largest case: 5 or 6) and three keys (the pairs with the next two
    contigs): 3 N - 3 keys, a longer list than any case's, every edge tile
    with edges."""
    c = np.arange(N, dtype=np.int64)
    m1, m2 = (1 + which, 1) if light else (3 + which, 1 + which)
    return cat(reads(c, None, m1), reads(c[:-1], c[:-1] + 1, m2), reads(c[:-2], c[:-2] + 2, 1))


def dirt_keys(N):
    return max(0, N) + max(0, N - 1) + max(0, N - 2)


def case(name, batch, N, bounds, rank=0, flagged=False, light_dirt=False, **kw):
    """An emulated-owner case: this process is `rank` of len(bounds) - 1 owners."""
    bounds = [int(x) for x in bounds]
    assert bounds[0] == 0 and bounds[-1] == N or len(bounds) == 2
    assert all(x <= y for x, y in zip(bounds, bounds[1:])) and 2 <= len(bounds) <= MAX_RUNS + 1
    n_loc = bounds[rank + 1] - bounds[rank]
    assert 1 <= n_loc <= 64, "this process's shard stays tiny"
    rec = records(batch, len(name))
    assert stays_deferred(rec, N)
    d = [dirt(N, 0, light_dirt), dirt(N, 1, light_dirt)]
    U = len(pair_list(batch)[0])
    assert dirt_keys(N) > U   # the dirtying lists are longer (their length: the CPU tests)
    return NS(name=name, batch=batch, rec=rec, N=int(N), bounds=bounds, rank=rank, n_loc=n_loc, flagged=flagged,
              dirt=d, U=U, **kw)


def chain_of(U, c0=37, step=1):
    """A chain whose list has exactly U keys, from contig c0."""
    if U == 0:
        return EMPTY
    p = (U - 1) // 2
    n = U - p
    ctg = c0 + step * np.arange(n, dtype=np.int64)
    pair = np.arange(n) < p
    b = chain(ctg, pair, 3, 2)
    assert len(pair_list(b)[0]) == U
    return b


def solo_bounds(N):
    return [0, 16]            # one owner: no exchange, the edge stage reads the records job's list


def three_bounds(N):
    return [0, 16, 16 + (N - 16) // 3, N]


@functools.lru_cache(maxsize=None)
def build_edge_len(U, W):
    b = chain_of(U)
    N = 37 + U + 9
    c = case(f"edge_len_{U}_w{W}", b, N, solo_bounds(N) if W == 1 else three_bounds(N))
    assert c.U == U
    return c


@functools.lru_cache(maxsize=None)
def build_edge_tiles(kind, W):
    if kind == "empty_tile":      # tile 1 holds diagonals only, tiles 0 and 2 hold edges
        n0 = ET // 2
        ctg = 20 + np.arange(n0 + ET + n0 + 1, dtype=np.int64)
        pair = np.r_[np.ones(n0, bool), np.zeros(ET, bool), np.ones(n0 + 1, bool)]
    elif kind == "diagonals_only":
        ctg = 20 + 3 * np.arange(ET + 77, dtype=np.int64)
        pair = np.zeros(len(ctg), bool)
    else:
        raise KeyError(kind)
    b = chain(ctg, pair, 2, 5)
    N = int(ctg[-1]) + 4
    c = case(f"edge_{kind}_w{W}", b, N, solo_bounds(N) if W == 1 else three_bounds(N))
    k, cnt = pair_list(b)
    m = graph([b], N)
    tiles = set((np.searchsorted(k, xr.key(m.a, m.b)) // ET).tolist())
    if kind == "empty_tile":
        assert tiles == {0, 2} and len(k) > 2 * ET
    else:
        assert len(m.a) == 0 and len(k) > ET
    return c


@functools.lru_cache(maxsize=None)
def build_second_round(edge_blocks=EDGE_BLOCKS, W=3):
    """More edge tiles than the edge stage's grid: the second grid-stride round
    runs and its tiles' prefix sums cross every tile of the first."""
    U = edge_blocks * ET + ET + 1
    b = chain_of(U, c0=5)
    N = 5 + U - (U - 1) // 2 + 3
    c = case("edge_second_round", b, N, solo_bounds(N) if W == 1 else three_bounds(N), edge_blocks=edge_blocks)
    assert -(-c.U // ET) > edge_blocks
    return c


@functools.lru_cache(maxsize=None)
def build_totals_fill(n_past, W):
    """Contigs before the first key, gaps of 1, 2 and 1,500 absent ids, n_past
    contigs past the last key."""
    step = [1, 2, 3, 1, 1501, 1, 2, 1501, 3, 1, 1, 2]
    ctg = 7 + np.cumsum(np.r_[0, np.tile(step, 4)])
    b = chain(ctg, True, 4, 3)
    N = int(ctg[-1]) + 1 + n_past
    c = case(f"totals_past_{n_past}_w{W}", b, N, solo_bounds(N) if W == 1 else three_bounds(N))
    m = graph([b], N)
    a = np.unique(xr.ab(pair_list(b)[0])[0])
    assert a[0] == 7 and {1, 2, 3, 1501} <= set(np.diff(a).tolist()) and N - 1 - a[-1] == n_past
    assert (m.totals == 0).sum() == N - len(ctg) and (m.totals == 0).sum() > 3000
    return c


@functools.lru_cache(maxsize=None)
def build_weights(W=3):
    """Repeated reads: shared counts and totals whose quotient a reciprocal
    multiply gets wrong.  (A count is a number of reads of the batch, so a
    count above 2^53, where int64 -> f64 rounds, cannot be reached from
    records; exchange_reference.build_weights covers that on graph.hip.)"""
    rng = np.random.default_rng(7)
    T = 400
    ctg = 30 + np.arange(T, dtype=np.int64)
    b = cat(chain(ctg, True, rng.integers(1, 60, T), rng.integers(1, 40, T)),
            reads(ctg[:-3], ctg[:-3] + 3, rng.integers(1, 25, T - 3)))
    N = 30 + T + 11
    c = case("weights", b, N, solo_bounds(N) if W == 1 else three_bounds(N))
    m = graph([b], N)
    differ = int(xr.recip_differs(m.shared, m.totals[m.a]).sum() + xr.recip_differs(m.shared, m.totals[m.b]).sum())
    assert differ >= 50 and not m.zero_div and m.shared.max() > 30
    c.recip_differ = differ
    return c


def owner_case(name, N, inner, pair=None, rank=0, flagged=False, light_dirt=False):
    """Every contig of [0, N) keyed (two keys each, one where pair is off); owner
    bounds 0, *inner, N."""
    ctg = np.arange(N, dtype=np.int64)
    b = chain(ctg, True if pair is None else pair, 2, 1)
    bounds = [0] + [int(x) for x in inner] + [N]
    c = case(name, b, N, bounds, rank, flagged, light_dirt)
    k, cnt, runs = owner_runs([b], bounds, N, 0)
    assert sum(runs) == c.U and len(runs) == len(bounds) - 1
    c.runs = runs
    c.geo = pr.geometry(N)
    return c


N_OWNERS = 70_001   # bw = 9, B = 137: buckets of 512 contigs, the last one partly filled


@functools.lru_cache(maxsize=None)
def build_ranks(W, flagged=False):
    """W owners: bounds on a bucket edge, inside a bucket, in the last bucket."""
    N = N_OWNERS
    g = pr.geometry(N)
    rng = np.random.default_rng(W)
    fixed = [16, 40 << g.bw, (77 << g.bw) + 5, ((g.B - 1) << g.bw) + 3][:W - 1]
    more = rng.choice(np.arange(17, N), max(0, W - 1 - len(fixed)), replace=False).tolist()
    inner = sorted(fixed + more)
    c = owner_case(f"ranks_{W}" + ("_flagged" if flagged else ""), N, inner, flagged=flagged)
    if W >= 5:
        bs = c.bounds[1:-1]
        assert any(x % (1 << g.bw) == 0 for x in bs) and any(x % (1 << g.bw) for x in bs)
        assert any((x >> g.bw) == g.B - 1 for x in bs) and (N >> g.bw) == g.B - 1
    assert all(bl.used == 0 for bl in windows(*_kr(c)))  # disjoint slices: every window is empty
    return c


def _kr(c):
    k, _, runs = owner_runs([c.batch], c.bounds, c.N, 0)
    return k, runs


@functools.lru_cache(maxsize=None)
def build_empty_owners():
    """Equal neighbouring bounds: empty owners first, in the middle and last
    (this process is owner 1: the first owner has no contig to hold), a bound
    at n_glob, and n_glob on a bucket edge (bd >> bw == B)."""
    g = pr.geometry(N_OWNERS)
    N = (g.B - 1) << g.bw
    assert (N >> pr.geometry(N).bw) == pr.geometry(N).B
    c = owner_case("empty_owners", N, [0, 16, 16, 5000, 5000, 5000, 30_000, N, N], rank=1)
    assert [i for i, x in enumerate(c.runs) if x == 0] == [0, 2, 4, 5, 8, 9]
    return c


@functools.lru_cache(maxsize=None)
def build_owner_slices():
    """Owners whose slices hold MT - 1, MT and MT + 1 keys (one tile less one, one tile, two tiles)."""
    h = MT // 2
    N = 16 + 3 * h + 1 + 200
    pair = np.ones(N, bool)
    pair[16 + h - 1] = False            # owner 1: h contigs, one of them a diagonal only
    pair[16 + 3 * h] = False            # owner 3: h + 1 contigs, one of them a diagonal only
    c = owner_case("owner_slices", N, [16, 16 + h, 16 + 2 * h, 16 + 3 * h + 1], pair)
    assert c.runs[1:4] == [MT - 1, MT, MT + 1]
    tiles = {}
    for bl in windows(*_kr(c)):
        tiles[bl.run] = tiles.get(bl.run, 0) + 1
    assert [tiles[r] for r in (1, 2, 3)] == [1, 1, 2]
    return c


@functools.lru_cache(maxsize=None)
def build_merge_stride(merge_blocks=8 * 256):
    """More merge tiles than the merge's grid (64 owners, 33 tiles each)."""
    W = MAX_RUNS
    per = -(-(merge_blocks + 1) // (W - 1))          # tiles per owner 1 .. W - 1
    n_own = per * MT // 2                            # contigs per owner: two keys each
    N = 16 + (W - 1) * n_own
    c = owner_case("merge_stride", N, [16 + n_own * i for i in range(W - 1)], light_dirt=True)
    assert sum(-(-x // MT) for x in c.runs) > merge_blocks
    c.merge_blocks = merge_blocks
    return c


EMU_CASES = {}
for _W in (1, 3):
    for _U in (0, 1, ET - 1, ET, ET + 1, 2 * ET + 1):
        EMU_CASES[f"edge_len_{_U}_w{_W}"] = (build_edge_len, (_U, _W))
    EMU_CASES[f"edge_empty_tile_w{_W}"] = (build_edge_tiles, ("empty_tile", _W))
    EMU_CASES[f"edge_diagonals_only_w{_W}"] = (build_edge_tiles, ("diagonals_only", _W))
    for _p in (1, 2, 5003):
        EMU_CASES[f"totals_past_{_p}_w{_W}"] = (build_totals_fill, (_p, _W))
    EMU_CASES[f"weights_w{_W}"] = (build_weights, (_W,))
for _W in (2, MFAST, MFAST + 1, MAX_RUNS):
    EMU_CASES[f"ranks_{_W}"] = (build_ranks, (_W,))
EMU_CASES["ranks_8_flagged"] = (build_ranks, (8, True))
EMU_CASES["empty_owners"] = (build_empty_owners, ())
EMU_CASES["owner_slices"] = (build_owner_slices, ())
# built with the device's grid caps by the GPU test: edge_second_round, merge_stride


def emu_case(name):
    f, args = EMU_CASES[name]
    return f(*args)


# ---- several ranks: the merge from slots ----------------------------------------------
def rank_case(name, W, bounds, batches, sizing=None, dirts=None, rerun=False):
    """batches[s]: rank s's reads of the deferred step under test.  sizing: the
    batches of the synchronous first step (default: the first dirtying step's)."""
    N = bounds[-1]
    assert len(bounds) == W + 1 == len(batches) + 1 and bounds[0] == 0 and W <= MFAST + 1
    assert all(16 <= y - x for x, y in zip(bounds, bounds[1:]))
    if dirts is None:
        dirts = [[dirt(N, 0)] * W, [dirt(N, 1)] * W]
    sizing = dirts[0] if sizing is None else sizing
    recs = [records(b, s + len(name)) for s, b in enumerate(batches)]
    for steps in (sizing, *dirts):
        for b in steps:
            assert stays_deferred(records(b, 1), N)
    assert all(stays_deferred(r, N) for r in recs)
    kc = slot_kc(sizing, bounds, N)
    for steps in dirts:
        assert max(max(s) for s in slices(steps, bounds, N)) <= kc
    mx = max(max(s) for s in slices(batches, bounds, N))
    assert (mx > kc) == rerun
    return NS(name=name, W=W, bounds=[int(x) for x in bounds], N=int(N), batches=batches, recs=recs, sizing=sizing,
              dirts=dirts, kc=kc, mx=mx, rerun=rerun)


def save_rank_case(c, path):
    """The .npz the child's rank threads load: records per rank and step."""
    d = {"bounds": np.array(c.bounds, np.int64), "rerun": np.array(c.rerun)}
    for s in range(c.W):
        d[f"sizing{s}"] = records(c.sizing[s], 11 + s)
        d[f"dirt0_{s}"] = records(c.dirts[0][s], 12 + s)
        d[f"dirt1_{s}"] = records(c.dirts[1][s], 13 + s)
        d[f"rec{s}"] = c.recs[s]
    np.savez(path, **d)


def owner_tiles(c, r=0):
    k, _, runs = owner_runs(c.batches, c.bounds, c.N, r)
    return windows(k, runs), runs


@functools.lru_cache(maxsize=None)
def build_ties(W):
    """The same reads on every rank (rank 0 holds one contig more, ahead of the
    rest): equal keys in every run; in owner 0's merged list one group of W
    equal keys lies across elements ET - 1 | ET."""
    n0 = 700
    bounds = [0, n0] + [n0 + 40 * s for s in range(1, W)]
    N = bounds[-1]
    rng = np.random.default_rng(W)
    ctg = np.arange(1, N, dtype=np.int64)
    same = chain(ctg, True, rng.integers(1, 9, N - 1), rng.integers(1, 9, N - 1))
    batches = [cat(reads([0]), same)] + [same] * (W - 1)
    c = rank_case(f"ties_{W}", W, bounds, batches)
    k, cnt, runs = owner_runs(batches, bounds, N, 0)
    mk, _ = merged_unsummed(k, cnt, runs)
    assert mk[ET - 1] == mk[ET] and (mk == mk[ET]).sum() == W and len(mk) > 2 * ET
    tiles, _ = owner_tiles(c)
    assert any(max(bl.lens) > 0 for bl in tiles) and all(bl.fast == (W <= MFAST) for bl in tiles)
    return c


def window_batches(lens_in, W, tail=60):
    """Owner 0: run 0's first tile holds the diagonals of contigs 0, 10, ..; run
    s >= 1 holds exactly lens_in[s - 1] diagonals inside that tile's key range.
    Past it every rank holds the same chain (ties, and the edges)."""
    assert len(lens_in) == W - 1
    span = 10 * (MT - 1)
    rng = np.random.default_rng(sum(lens_in) + W)
    zone = span + 1 + np.arange(tail, dtype=np.int64)
    n0 = span + 1 + tail + 3
    bounds = [0, n0] + [n0 + 20 * s for s in range(1, W)]
    common = chain(np.r_[zone, np.arange(n0, bounds[-1])], True, 2, 3)
    batches = [cat(reads(10 * np.arange(MT)), common)]
    for j, ln in enumerate(lens_in):
        inside = np.sort(rng.choice(span, ln, replace=False)) if j else np.arange(ln)
        batches.append(cat(reads(inside), common))
    return bounds, batches


@functools.lru_cache(maxsize=None)
def build_window(lens_in, slow_tile0=False):
    W = len(lens_in) + 1
    bounds, batches = window_batches(lens_in, W)
    c = rank_case("window_" + "_".join(map(str, lens_in)), W, bounds, batches)
    tiles, runs = owner_tiles(c)
    bl = tiles[0]
    assert (bl.run, bl.tile) == (0, 0) and bl.lens[1:] == list(lens_in) and runs[0] > MT
    used, staged = 0, []
    for s, ln in enumerate(lens_in, 1):
        if used + ln <= MLDS:
            staged.append(s)
            used += ln
    assert bl.staged == staged and bl.used == used
    # one window: the fast path is left by that tile only.  (With more runs a
    # later run's tile that spans the spilled run's keys leaves it as well.)
    slow = [(t.run, t.tile) for t in tiles if not t.fast]
    assert bl.fast == (not slow_tile0) and (len(lens_in) > 1 or slow == [(0, 0)][:int(slow_tile0)])
    for r in range(1, W):
        assert all(t.fast for t in owner_tiles(c, r)[0])
    c.slow_tiles = slow
    return c


@functools.lru_cache(maxsize=None)
def build_world9():
    """Nine runs: no tile takes the fast path; windows are non-empty, keys tie."""
    c9 = build_ties(MFAST + 1)
    tiles, _ = owner_tiles(c9)
    assert not any(bl.fast for bl in tiles) and all(not bl.inplace for bl in tiles)
    return c9


@functools.lru_cache(maxsize=None)
def build_run_lengths():
    """Owner 0 receives 0, 1, MT - 1, MT, MT + 1 keys and 0 again; owner 6 receives nothing from anyone."""
    W = 7
    n0 = MT + 40
    bounds = [0, n0] + [n0 + 30 * s for s in range(1, W)]
    others = chain(np.arange(n0, bounds[W - 1]), True, 3, 2)      # owners 1 .. 5; nothing for owner 6
    want = [0, 1, MT - 1, MT, MT + 1, 0, 3]
    batches = [cat(reads(5 + np.arange(n)), others) for n in want]
    c = rank_case("run_lengths", W, bounds, batches)
    sl = slices(batches, bounds, c.N)
    assert [s[0] for s in sl] == want and all(s[W - 1] == 0 for s in sl)
    return c


@functools.lru_cache(maxsize=None)
def build_run_touch():
    """Owner 0's runs touch at a tile edge inside run 1 (two tiles): the last key
    of its first tile is the first key of run 0, an earlier run that reaches
    past it; the first key of its second tile is the last key of run 2, a later
    run that starts before it.  Neither run is wholly before or after those
    keys, and only the tile's side takes the shortcut.  (Where two runs touch
    end to end, swapping <= and < in the shortcut flips the tie on both sides
    and only swaps two equal keys: no output changes.)"""
    W, c0 = 3, 100
    edge = c0 + MT - 1                       # the contig of run 1's element MT - 1
    n0 = edge + 240
    bounds = [0, n0, n0 + 20, n0 + 40]
    tail = chain(np.arange(n0, bounds[-1]), True, 2, 2)
    batches = [cat(reads(np.arange(edge, edge + 180)), tail), cat(reads(np.arange(c0, edge + 80)), tail),
               cat(reads(np.arange(edge - 120, edge + 2)), tail)]
    c = rank_case("run_touch", W, bounds, batches)
    k, _, runs = owner_runs(batches, bounds, c.N, 0)
    off = np.r_[0, np.cumsum(runs)]
    assert MT < runs[1] <= 2 * MT and runs[0] <= MT and runs[2] <= MT
    last0, first1 = k[off[1] + MT - 1], k[off[1] + MT]            # run 1's tile edge
    assert last0 == k[off[0]] and k[off[1] - 1] > last0           # run 0 starts there and goes on
    assert first1 == k[off[3] - 1] and k[off[2]] < first1         # run 2 ends there and starts earlier
    return c


@functools.lru_cache(maxsize=None)
def build_slot(extra):
    """The sizing step leaves room for kc keys; rank 1's slice for owner 0 holds kc + extra."""
    W = 3
    small = chain(np.arange(0, 100), True, 2, 1)
    kc = 199 + 199 // 4 + 1024
    n0 = kc + 30
    bounds = [0, n0, n0 + 20, n0 + 40]
    sizing = [small] * W
    assert slot_kc(sizing, bounds, bounds[-1]) == kc
    d0 = [chain(np.arange(0, 300), True, 70, 3)] * W
    d1 = [chain(np.arange(0, bounds[-1], 2), False, 80, 1)] * W
    tail = chain(np.arange(n0, bounds[-1]), True, 2, 2)
    batches = [cat(small, tail), cat(reads(np.arange(kc + extra)), tail), cat(chain(np.arange(50, 90), True), tail)]
    c = rank_case(f"slot_kc_plus_{extra}", W, bounds, batches, sizing, [d0, d1], rerun=extra > 0)
    assert c.kc == kc and c.mx == kc + extra
    return c


RANK_CASES = {
    "ties_2": (build_ties, (2,)),
    "ties_3": (build_ties, (3,)),
    "ties_8": (build_ties, (8,)),
    "world_9": (build_world9, ()),
    "window_small": (build_window, ((0, 1, 2, 3, 4, 7, 8),)),
    "window_pow2": (build_window, ((15, 16, 31, 32, 63, 64, 127),)),
    "window_pow2_large": (build_window, ((128, 255, 256, 511, 512, 1023, 1024),)),
    "window_1_and_5000": (build_window, ((1, 5000),)),
    "window_lds_minus_1": (build_window, ((MLDS - 1,),)),
    "window_lds": (build_window, ((MLDS,),)),
    "window_lds_plus_1": (build_window, ((MLDS + 1,), True)),
    "window_two_halves_over": (build_window, ((MLDS // 2, MLDS // 2 + 1), True)),
    "window_spill_then_small": (build_window, ((MLDS + 1, 10), True)),
    "run_lengths": (build_run_lengths, ()),
    "run_touch": (build_run_touch, ()),
    "slot_kc": (build_slot, (0,)),
    "slot_kc_plus_1": (build_slot, (1,)),
}


def rank_case_named(name):
    f, args = RANK_CASES[name]
    return f(*args)
