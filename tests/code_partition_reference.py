"""Inputs that put the records graph's code-partition path on its limits
(graph_sets.hip: partition_kernel<CodeStream>, code_append_kernel,
code_reduce_kernel through stream_runs; their arithmetic: csrc/code_part.h).
No device calls here: tests/test_code_partition_reference_cpu.py checks every
builder against its own placement and the plain model (pairs_reference.
pair_graph) against the oracle; tests/test_gpu_code_partition.py runs the
inputs, with the geometry the library reports.

How an input is placed.  With KARMA_CHUNK=2048 classify chunk c covers records
[2048 c, 2048 (c + 1)) and writes the compact codes of the reads that START in
it to its own list (classify2_kernel: `out = P.codes + c_lo`, one wave per
chunk; a read that starts in a chunk is emitted by that chunk's wave).  No read
built here crosses a chunk, so a chunk's list holds exactly the codes of its
reads, in an order the kernel chooses.  A partition block takes `lpb`
consecutive lists as one range and flushes it `flush` codes at a time (8,192 =
4 chunks, 12,288 = 6 chunks): as long as every chunk before a flush boundary
is full of one-record compact reads, the boundary falls between two lists and
a flush's per-bucket histogram does not depend on the order inside a list.
placement() recomputes the histograms from the records alone and insists on
that.

A compact read here is one record (read r hits contig m0 < N - 3 only; its
code is m0_local << 3 | 0 in code bucket m0 >> bwc; where a chunk has one
record left over, its last read takes two, {m0, m0 + 1}: code m0_local << 3 |
1).  Records that must yield no code are big reads (more than 8 records, the
separate generic path) of 32 records or more: the relabel probe counts a
32-record window only when a read starts and ends inside it, so such reads
keep it quiet, where chunks of general reads would call for the relabelled
rerun and move every code to another bucket.
"""
import types

import numpy as np

import pairs_reference as pr

CHUNK = 2048          # records per classify chunk (the smallest KARMA_CHUNK takes)
# csrc/code_part.h, restated (test_code_partition_reference_cpu.py compares them with the header)
CODE_FILL = 8192      # kCodeFill: codes per flush of partition_kernel<CodeStream>
APPEND_CAP = 12288    # kAppendCap: codes per flush of code_append_kernel
MAX_LISTS = 128       # kMaxListsPerBlock
NARROW_BC, APPEND_MIN_BC, MAX_BC = 128, 129, 512
CR_PIECES, CR_SMAX, CG_SHIFT = 512, 64, 18
ROUND_VECS = 64 * 16  # 16-byte vectors of one stream_runs round of a wave (64 x kWin)


def geometry(n_contigs, n_chunks, lpb, path=None):
    """The fields of karma_graph_code_geometry a builder needs, by hand (CPU
    tests; the GPU tests pass _lib.code_geometry's result instead)."""
    g = pr.geometry(n_contigs)
    path = path if path is not None else (3 if g.Bc >= APPEND_MIN_BC else 2)
    return types.SimpleNamespace(Bc=g.Bc, bwc=g.bwc, chunk=CHUNK, n_chunks=n_chunks, path=path, lpb=lpb,
                                 n_pblk=-(-n_chunks // lpb), flush={2: CODE_FILL, 3: APPEND_CAP}[path])


def reduce_split(R):
    """code_part.h reduce_split: pieces a directory row's run is read in."""
    return max(1, min(CR_SMAX, -(-CR_PIECES // R))) if R > 0 else 1


def staged(hists):
    """code_append_kernel's staged codes per flush of one block (code_part.h
    flush_scan): the sum over buckets of roundup8(pending + new)."""
    pc = np.zeros(len(hists[0]), np.int64)
    out = []
    for h in hists:
        tot = pc + np.asarray(h, np.int64)
        out.append(int(((tot + 7) & ~7).sum()))
        pc = tot & 7
    return out


def staged_bound(cap, nb):
    return 16 * nb + ((cap - 2 * nb) & ~7) if cap >= 2 * nb else 8 * nb + 8 * (cap // 2)


# ---- records from histograms -----------------------------------------------------------
def _filler(k, n_contigs, at):
    """k >= 2 records that yield no code: big reads of 32 to 63 records on
    consecutive contigs (one read of k records when k < 32; a general read on
    every fourth contig when k < 9), starting at contigs rising from `at`."""
    assert k >= 2
    sizes = [k] if k < 64 else [32] * (k // 32 - 1) + [32 + k % 32]
    ctg, rid = [], []
    for i, s in enumerate(sizes):
        a = (at + 7 * i) % (n_contigs - 64)
        ctg.append(a + np.arange(s) * (4 if s < 9 else 1))
        rid.append(np.full(s, i))
    return np.concatenate(ctg), np.concatenate(rid)


def build(geo, n_contigs, blocks, seed=0, m0=None):
    """Records whose partition block k has the per-flush, per-bucket code
    histograms blocks[k] (a list of arrays of geo.Bc counts; [] or all-zero: a
    block with no item).  Every flush but a block's last holds geo.flush codes.
    Every block but the last spans geo.lpb chunks; what its codes do not fill
    are chunks of big reads (empty lists).  The last block ends with its
    last chunk that holds a code (or spans one chunk if it has none), unless
    `geo.n_chunks` asks for more.  m0(bucket, k) gives the contigs of k codes
    of a bucket (default: seeded random ones inside it)."""
    rng = np.random.default_rng(seed)
    width = 1 << geo.bwc
    assert geo.flush % CHUNK == 0 and len(blocks) == geo.n_pblk

    def contigs(b, k):
        lo, hi = b * width, min((b + 1) * width, n_contigs - 3)
        assert lo < hi, "bucket %d holds no contig below N - 3" % b
        return rng.integers(lo, hi, k) if m0 is None else np.asarray(m0(b, k), np.int64)

    ctg_all, rid_all = [], []
    for k, flushes in enumerate(blocks):
        last_block = k == len(blocks) - 1
        codes = []
        for f, h in enumerate(flushes):
            h = np.asarray(h, np.int64)
            assert len(h) == geo.Bc and (h >= 0).all()
            assert h.sum() == geo.flush or (f == len(flushes) - 1 and h.sum() <= geo.flush), (k, f, int(h.sum()))
            c = np.concatenate([contigs(b, int(h[b])) for b in np.flatnonzero(h)]) if h.sum() else np.zeros(0, np.int64)
            codes.append(rng.permutation(c))
        codes = np.concatenate(codes) if codes else np.zeros(0, np.int64)
        full, part = divmod(len(codes), CHUNK)
        used = full + (1 if part else 0)
        n_ch = geo.lpb if not last_block else max(1, used, geo.n_chunks - geo.lpb * k)
        assert used <= n_ch <= geo.lpb, "block %d: %d chunks of codes, %d lists" % (k, used, geo.lpb)
        rid = np.arange(len(codes))
        if part == CHUNK - 1:  # no room for a general read: the last code's read takes two records, {m0, m0 + 1}
            codes, rid, part = np.r_[codes, codes[-1] + 1], np.r_[rid, rid[-1]], 0
        ctg_all.append(codes)
        rid_all.append(rid)
        # the partial chunk's rest, then whole chunks: no general read crosses a chunk
        for k_fill in ([CHUNK - part] if part else []) + [CHUNK] * (n_ch - used):
            gc, gr = _filler(k_fill, n_contigs, int(rng.integers(0, n_contigs - 64)))
            ctg_all.append(gc)
            rid_all.append(gr)
    # read ids in record order, grouped and rising
    ctg = np.concatenate(ctg_all)
    change = np.concatenate([np.r_[True, r[1:] != r[:-1]] for r in rid_all if len(r)])
    rec = np.stack([np.cumsum(change) - 1, ctg], 1).astype(np.uint32)
    assert len(rec) == geo.n_chunks * CHUNK, (len(rec), geo.n_chunks)
    got = placement(rec, n_contigs, geo)
    want = [[np.asarray(h, np.int64) for h in fl if np.asarray(h).sum()] for fl in blocks]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)), "the records miss their placement"
    assert not pr.relabels(rec, n_contigs), "the relabel probe would fire"
    return rec


def placement(rec, n_contigs, geo):
    """Per partition block, the per-flush code-bucket histograms the records give,
    from the records alone; fails if a flush boundary falls inside a chunk's
    list (the order inside a list is the kernel's)."""
    rec = np.asarray(rec, np.int64)
    off = pr.read_bounds(rec)
    ctg = rec[:, 1]
    lo = np.minimum.reduceat(ctg, off[:-1])
    hi = np.maximum.reduceat(ctg, off[:-1])
    n_rec = np.diff(off)
    assert ((off[:-1] // CHUNK) == ((off[1:] - 1) // CHUNK)).all(), "a read crosses a chunk"
    compact = (hi - lo <= 3) & (n_rec <= 8)  # big reads (the filler) yield no code
    assert (lo[compact] < n_contigs - 3).all() and (hi < n_contigs).all()
    chunk_of = off[:-1][compact] // CHUNK
    bucket = lo[compact] >> geo.bwc
    n_chunks = -(-len(rec) // CHUNK)
    out = []
    for k in range(-(-n_chunks // geo.lpb)):
        c0, c1 = k * geo.lpb, min((k + 1) * geo.lpb, n_chunks)
        sel = (chunk_of >= c0) & (chunk_of < c1)
        per_list = np.bincount(chunk_of[sel] - c0, minlength=c1 - c0)
        cum = np.r_[0, np.cumsum(per_list)]
        items = int(cum[-1])
        live = np.flatnonzero(per_list)
        assert (cum[live] // geo.flush == (cum[live + 1] - 1) // geo.flush).all(), \
            "block %d: a flush boundary inside a list" % k
        flush_of = cum[chunk_of[sel] - c0] // geo.flush
        fl = [np.bincount(bucket[sel][flush_of == f], minlength=geo.Bc) for f in range(-(-items // geo.flush))]
        assert all(h.sum() == min(geo.flush, items - f * geo.flush) for f, h in enumerate(fl))
        out.append(fl)
    return out


# ---- histograms ------------------------------------------------------------------------
def spread(n, nb, base=None, to=0):
    """n codes over nb buckets: base[b] each (default 0), the rest to bucket `to`."""
    h = np.zeros(nb, np.int64) if base is None else np.array(base, np.int64)
    assert h.sum() <= n
    h[to] += n - h.sum()
    return h


def usable(geo, n_contigs):
    """Leading code buckets that hold a contig below N - 3 (the last bucket of
    N = 2^k + 1 holds one contig: it exists, and no read built here reaches it)."""
    u = int(np.count_nonzero((np.arange(geo.Bc) << geo.bwc) < n_contigs - 3))
    assert u >= geo.Bc - 1
    return u


def pad(h, geo):
    return np.r_[np.asarray(h, np.int64), np.zeros(geo.Bc - len(h), np.int64)]


def random_hist(rng, n, geo, u, live=None):
    """n codes at random over the first `live` (default: all usable) buckets."""
    return pad(np.bincount(rng.integers(0, live or u, n), minlength=u), geo)


def worst_case_regions(geo, u):
    """Two flushes of code_append_kernel that stage the most codes a flush can
    over u buckets (code_part.h staged_bound): flush 1 leaves 7 pending codes in
    every bucket (one bucket fewer unless 8 divides u: a full flush leaves a
    multiple of 8 pending in all), flush 2 brings each bucket the fewest codes
    that put its total at 1 (mod 8), and whole eights to bucket 0."""
    cap = geo.flush
    h1 = np.full(u, 7, np.int64)
    rest = cap - h1.sum()
    h1[0] += rest & ~7
    h1[-1] += rest & 7
    h2 = (1 - h1) & 7
    h2[0] += (cap - h2.sum()) & ~7
    assert h1.sum() == cap and h2.sum() <= cap
    assert staged([h1, h2])[1] == staged_bound(cap, u)
    return [pad(h1, geo), pad(h2, geo)]


# ---- cases: name -> (n_contigs, chunks, KARMA_PART_RESIDENT or None, blocks(geo, u, rng)) ------
# `chunks` may be a function of the flush size in chunks (4 or 6).  The blocks
# are made from the geometry the library reports (GPU tests) or geometry() by
# hand (CPU tests): lpb, n_pblk and flush are never literals here.
PATH2_N = (3648, 4096, 262145, 524288)        # 57, 64, 65 (bwc 12, a second scan group of one) and 128 buckets
PATH3_N = (524289, 1200129, 1600000, 1 << 21)  # 129, 294, 391 and 512 buckets


def _items_case(items_of):
    """Two blocks: block 0 holds items_of(cap) codes (then empty lists), block 1
    one flush and 1,234 codes."""
    def blocks(geo, u, rng):
        out = []
        for items in (items_of(geo.flush), geo.flush + 1234):
            out.append([random_hist(rng, min(geo.flush, items - b), geo, u) for b in range(0, items, geo.flush)])
        return out
    return blocks


def _items_chunks(items_of):
    # both blocks span lpb = the chunks the larger one needs
    return lambda per: 2 * max(-(-items_of(per * CHUNK) // CHUNK), per + 1)


ITEMS = {"cap-1": lambda c: c - 1, "cap": lambda c: c, "cap+1": lambda c: c + 1, "2cap": lambda c: 2 * c,
         "2cap+1": lambda c: 2 * c + 1}


def _one_bucket(geo, u, rng):
    # every code of a flush in one bucket: ranks up to flush - 1 in the packed 16-bit ranks
    return [[spread(geo.flush, geo.Bc, to=u // 2), spread(geo.flush, geo.Bc, to=u - 1), spread(5, geo.Bc, to=0)]]


def _mod8_one(geo, u, rng):
    # every usable bucket's count = 1 (mod 8): the most padding a flush holds
    h = pad(1 + 8 * rng.integers(0, 3, u), geo)
    full = pad(np.ones(u, np.int64), geo)
    full[1] += (geo.flush - u) & ~7
    return [[h]] if (geo.flush - u) % 8 else [[full, h]]


def _residues(geo, u, rng):
    # per-bucket counts of every residue mod 8 over three flushes; buckets from 3 u / 4 on hold no code
    live = 3 * u // 4
    fl = []
    for f in range(3):
        h = pad((np.arange(live) + 3 * f) % 8, geo)
        fl.append(spread(geo.flush if f < 2 else int(h.sum()) + 13, geo.Bc, base=h, to=(5 * f) % live))
    return [fl]


def _holes(geo, u, rng):
    # empty lists inside a block, a block with no item, the last block empty
    return [[random_hist(rng, 700, geo, u)], [], [random_hist(rng, geo.flush, geo, u), random_hist(rng, 3, geo, u)], []]


def _lists(geo, u, rng):
    # every chunk full of codes: lpb lists a block (128 with 128 chunks or more)
    out, left = [], geo.n_chunks * CHUNK
    for k in range(geo.n_pblk):
        items = min(left, geo.lpb * CHUNK)
        out.append([random_hist(rng, min(geo.flush, items - b), geo, u) for b in range(0, items, geo.flush)])
        left -= items
    return out


def _round(delta):
    # one block, one flush, one directory row read as 64 pieces: bucket 1's run
    # is one stream_runs round of vectors (8 codes each) + delta; 2,000 codes
    # in the buckets from 2 on
    def blocks(geo, u, rng):
        other = np.r_[0, 0, np.bincount(rng.integers(0, u - 2, 2000), minlength=u - 2)]
        other[1] = 8 * (ROUND_VECS + delta)
        assert other.sum() <= geo.flush
        return [[pad(other, geo)]]
    return blocks


def _worst(geo, u, rng):
    return [worst_case_regions(geo, u)]


CASES = {}
for _n in PATH2_N + PATH3_N:
    for _k, _f in ITEMS.items():
        CASES["items_%s_n%d" % (_k, _n)] = (_n, _items_chunks(_f), 2, _items_case(_f))
    CASES["one_bucket_n%d" % _n] = (_n, lambda per: 2 * per + 1, 1, _one_bucket)
    CASES["holes_n%d" % _n] = (_n, lambda per: 4 * (per + 1) - 1, 4, _holes)
    CASES["residues_n%d" % _n] = (_n, lambda per: 3 * per, 1, _residues)
for _n in PATH2_N:
    CASES["mod8_one_n%d" % _n] = (_n, lambda per: 2 * per, 1, _mod8_one)
for _n in (3648, 524288, 524289):
    CASES["lists_128_n%d" % _n] = (_n, lambda per: 128, 1, _lists)
    CASES["lists_129_n%d" % _n] = (_n, lambda per: 129, 1, _lists)
for _n in PATH3_N[1:]:
    CASES["worst_case_regions_n%d" % _n] = (_n, lambda per: 2 * per, 1, _worst)
for _d in (-1, 0, 1):
    CASES["round_%+d_n524289" % _d] = (524289, lambda per: 5, 1, _round(_d))
# directory rows R = blocks of one list each (no KARMA_PART_RESIDENT): S = 64, 64, 57 at
# 129 buckets (runs of ~2 vectors and of 0: shorter than S), 2, 1, 1 at 57 buckets
for _n, _rows in ((524289, (1, 8, 9)), (3648, (511, 512, 513))):
    for _r in _rows:
        CASES["rows_%d_n%d" % (_r, _n)] = (_n, (lambda r: lambda per: r)(_r), None, _lists)


def case_geometry(name, per_of_path={2: CODE_FILL // CHUNK, 3: APPEND_CAP // CHUNK}):
    """(n_contigs, chunks, knob) of a case; the flush size in chunks from the path make_geo gives."""
    n, chunks, knob, _ = CASES[name]
    path = 3 if pr.geometry(n).Bc >= APPEND_MIN_BC else 2
    return n, chunks(per_of_path[path]), knob


def case_records(name, geo):
    """The case's records for the geometry `geo` (of case_geometry's shape)."""
    n = CASES[name][0]
    rng = np.random.default_rng(sum(name.encode()))
    return build(geo, n, CASES[name][3](geo, usable(geo, n), rng), seed=len(name))


def shuffled_ids(n_contigs, A, seed=3):
    """Compact reads of 1 to 4 records, each on contigs of its own (read i within
    [4 i, 4 i + 4)), whose contig ids went through a random permutation: reads
    span the whole range and the relabel probe fires.  The relabelling groups
    contigs that share a read (SetsJob::relabel: each contig is hooked to the
    smallest one it shares a read with, contigs are renumbered root by root),
    and no contig is shared between reads here, so the relabelled rerun finds
    every read compact again: no general read, no full pair list, two attempts."""
    rng = np.random.default_rng(seed)
    assert 4 * A <= n_contigs - 3
    m0 = 4 * np.arange(A)
    M = rng.integers(0, 8, A)
    hit = np.concatenate([np.ones((A, 1), bool), ((M[:, None] >> np.arange(3)) & 1).astype(bool)], 1)
    contig = (m0[:, None] + np.arange(4))[hit]
    read = np.broadcast_to(np.arange(A)[:, None], hit.shape)[hit]
    perm = rng.permutation(n_contigs)
    return np.stack([read, perm[contig]], 1).astype(np.uint32)[:A]
