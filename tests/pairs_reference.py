"""A plain model of the records graph and inputs that sit on the capacities of
its pair-bucket stage (graph_sets.hip: general_kernel, the pair partition,
pair_reduce_kernel, final_kernel<4096 | 8192>, bucket_widen_kernel,
assemble2_kernel).  No device calls here: tests/test_pairs_reference_cpu.py
checks the model against the oracle and every builder against its own
condition; tests/test_gpu_pair_buckets.py runs the builders' inputs.

The model is written from the definition: a read's set of
contigs gives every pair (a <= b) of that set, the diagonal included; the
list is the sorted keys a << 32 | b with their counts; an edge is a pair a < b
with weight (s / ta + s / tb) / 2, one IEEE operation each.

What the builders restate of the device code, so that an input lands where it
is meant to (each restated rule is checked against the kernels' results by the
GPU tests' launch counts, never assumed):
  * make_geo                  -> geometry()
  * relabel_probe_kernel      -> probe_wide_windows()
  * a chunk's general reads   -> chunk_pairs()  (a read belongs to the chunk it
                                 starts in; <= 8 records; contigs span > 3 ids)
"""
import functools
import types

import numpy as np

CHUNK = 4096          # records per classify chunk of small inputs (chunk_records)
HASH_R = 4096         # pair_reduce_kernel's hash slots
HASH_R_FILL = HASH_R - HASH_R // 8   # 3584: more distinct keys hand the bucket to the generic path
HASH_F = 8192         # final_kernel<8192>'s hash slots (merged flush groups)
BAND = 8192           # band counters per bucket
PROBES, PROBE_W = 256, 32


# ---- the model ----------------------------------------------------------------------
def read_bounds(records):
    """Starts of the reads of grouped records (runs of one read id), and the end."""
    rec = np.asarray(records, np.int64).reshape(-1, 2)
    if not len(rec):
        return np.zeros(1, np.int64)
    return np.r_[np.flatnonzero(np.r_[True, rec[1:, 0] != rec[:-1, 0]]), len(rec)]


def pair_graph(records, n_contigs):
    rec = np.asarray(records, np.int64).reshape(-1, 2)
    off = read_bounds(rec).tolist()
    ctg = rec[:, 1].tolist()
    counts = {}
    for r in range(len(off) - 1):
        s = sorted(set(ctg[off[r]:off[r + 1]]))
        for i, a in enumerate(s):
            for b in s[i:]:
                k = a << 32 | b
                counts[k] = counts.get(k, 0) + 1
    keys = np.array(sorted(counts), np.uint64)
    cnt = np.array([counts[int(k)] for k in keys], np.int64)
    a = (keys >> np.uint64(32)).astype(np.int64)
    b = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    totals = np.zeros(n_contigs, np.int64)
    diag = a == b
    totals[a[diag]] = cnt[diag]
    e = ~diag
    s = cnt[e].astype(np.float64)
    ta = totals[a[e]].astype(np.float64)
    tb = totals[b[e]].astype(np.float64)
    weight = (s / ta + s / tb) / 2.0
    return types.SimpleNamespace(keys=keys, counts=cnt, totals=totals, a=a[e].astype(np.uint32),
                                 b=b[e].astype(np.uint32), shared=cnt[e], weight=weight)


def geometry(n_contigs):
    """make_geo restated."""
    N = int(n_contigs)
    assert 1 <= N <= 1 << 24
    bbits = 1
    while (1 << bbits) < N:
        bbits += 1
    nb = lambda w: (N + (1 << w) - 1) >> w
    bw = 4
    while nb(bw) > 256 and bw < 10:
        bw += 1
    while nb(bw) > 2048:
        bw += 1
    B = nb(bw)
    dbits = 3 if bw + 3 <= 13 else (13 - bw if bw <= 13 else -1)
    bwc, Bc = (bw + 2, nb(bw + 2)) if bw <= 10 else (0, 0)
    n_pg = 1 if B >= 128 else -(-256 // B)
    return types.SimpleNamespace(bw=bw, bbits=bbits, B=B, dbits=dbits, bwc=bwc, Bc=Bc, n_pg=n_pg)


# ---- what an input does to the stage, counted with the model --------------------------
def hash_pairs_per_bucket(records, n_contigs, lo=0, hi=None):
    """{bucket: distinct pairs with b - a >= 8} of the general reads that start in
    records [lo, hi): the keys pair_reduce_kernel hashes."""
    g = geometry(n_contigs)
    out = {}
    for s in general_reads(records, lo, hi):
        for i, a in enumerate(s):
            for b in s[i:]:
                if b - a >= (1 << g.dbits):
                    out.setdefault(a >> g.bw, set()).add((a, b))
    return {k: len(v) for k, v in out.items()}


def general_reads(records, lo=0, hi=None):
    """Sorted contig sets of the reads on the general path (<= 8 records, span > 3)
    that start in records [lo, hi)."""
    rec = np.asarray(records, np.int64).reshape(-1, 2)
    off = read_bounds(rec).tolist()
    ctg = rec[:, 1].tolist()
    hi = len(rec) if hi is None else hi
    for r in range(len(off) - 1):
        if not lo <= off[r] < hi or off[r + 1] - off[r] > 8:
            continue
        s = sorted(set(ctg[off[r]:off[r + 1]]))
        if s[-1] - s[0] > 3:
            yield s


def big_reads(records):
    off = read_bounds(records)
    return int((np.diff(off) > 8).sum())


def chunk_pairs(records, chunk=CHUNK):
    """Pairs general_kernel writes per chunk: u (u + 1) / 2 per general read."""
    A = len(records)
    return [sum(len(s) * (len(s) + 1) // 2 for s in general_reads(records, c, c + chunk))
            for c in range(0, max(A, 1), chunk)]


def flush_groups(records, n_contigs, chunk=CHUNK):
    """Record ranges [lo, hi) of the pair reduce's flush groups, for inputs whose
    chunks each fit one pair flush (<= 4,096 pairs, one chunk list per partition
    block): flush f is the f-th chunk with pairs, group_range splits them evenly."""
    cp = chunk_pairs(records, chunk)
    assert max(cp) <= 4096
    fl = [c for c, p in enumerate(cp) if p]
    n_pg = geometry(n_contigs).n_pg
    per = -(-len(fl) // n_pg)
    return [(fl[g * per] * chunk, (fl[min(len(fl), (g + 1) * per) - 1] + 1) * chunk)
            for g in range(n_pg) if g * per < len(fl)]


def band_slots(records, n_contigs, bucket):
    """Nonzero band counters (a_local, b - a < 8) of a bucket."""
    g = geometry(n_contigs)
    m = pair_graph(records, n_contigs)
    a = (m.keys >> np.uint64(32)).astype(np.int64)
    d = (m.keys & np.uint64(0xFFFFFFFF)).astype(np.int64) - a
    return int(((a >> g.bw == bucket) & (d < (1 << g.dbits))).sum())


def probe_wide_windows(records, n_contigs):
    """relabel_probe_kernel restated: 256 evenly spaced windows of 32 records from an
    even position; a window counts when the first read that starts and ends inside
    it spans more than 4 ids.  More than 32 ask for the relabelled rerun."""
    rec = np.asarray(records, np.int64).reshape(-1, 2)
    A, wide = len(rec), 0
    for t in range(PROBES):
        p = (A * t // PROBES) & ~1
        if p + PROBE_W > A:
            continue
        rid, ctg = rec[p:p + PROBE_W, 0], rec[p:p + PROBE_W, 1]
        starts = [j for j in range(1, PROBE_W) if rid[j] != rid[j - 1]]
        if len(starts) >= 2:
            c = ctg[starts[0]:starts[1]]
            if c.max() - c.min() > 3 and c.max() < n_contigs:
                wide += 1
    return wide


def relabels(records, n_contigs):
    return probe_wide_windows(records, n_contigs) * 8 > PROBES


# ---- layout -------------------------------------------------------------------------
def lay_out(chunks, filler, chunk=CHUNK):
    """Records of len(chunks) whole chunks: chunk c holds the reads chunks[c] (lists
    of contigs, every read inside its chunk), every other record is a read of its
    own on the next contig of `filler` (one code, no pair list entry).  No placed
    read covers the record after a probe position, so each probe window's first
    read is a filler read and the relabel probe stays quiet."""
    A = len(chunks) * chunk
    after_probe = np.zeros(A + 16, bool)
    for t in range(PROBES):
        after_probe[((A * t // PROBES) & ~1) + 1] = True
    ctg = np.full(A, -1, np.int64)
    rid = np.zeros(A, np.int64)
    nxt = 1
    for c, reads in enumerate(chunks):
        pos = c * chunk
        for read in reads:
            L = len(read)
            while after_probe[pos:pos + L].any():
                pos += 1
            assert pos + L <= (c + 1) * chunk, "reads do not fit their chunk"
            ctg[pos:pos + L] = read
            rid[pos:pos + L] = nxt
            nxt += 1
            pos += L
    free = np.flatnonzero(ctg < 0)
    ctg[free] = np.resize(np.asarray(filler, np.int64), len(free))
    rid[free] = nxt + np.arange(len(free))
    # read ids in record order (grouped and rising, as a sorted file has them)
    first = np.r_[True, rid[1:] != rid[:-1]]
    return np.stack([np.cumsum(first) - 1, ctg], 1).astype(np.uint32)


def spread(reads, budget, n_chunks=None):
    """The reads in order over the fewest chunks (or n_chunks) with at most `budget`
    pairs each, evenly."""
    cost = [len(set(r)) * (len(set(r)) + 1) // 2 if max(r) - min(r) > 3 else 0 for r in reads]  # general reads only
    n = n_chunks or max(1, -(-sum(cost) // budget))
    while True:
        parts = [list(p) for p in np.array_split(np.arange(len(reads)), n)]
        if all(sum(cost[i] for i in p) <= budget for p in parts):
            return [[reads[i] for i in p] for p in parts]
        assert n_chunks is None, "the reads do not fit the chunks asked for"
        n += 1


def interleave(many, few):
    """`few` at even distances among `many`."""
    out, step = [], len(many) / max(1, len(few))
    for i, r in enumerate(few):
        out += many[int(i * step):int((i + 1) * step)] + [r]
    return out + many[int(len(few) * step):]


def hash_reads(base, n, b0):
    """General reads with exactly n distinct pairs (a, b), b - a >= 8, a in
    [base, base + 16): reads of 4 + 4 contigs (16 pairs each, 36 list entries) and
    up to two smaller ones for n % 16.  b starts at b0 >= base + 23; the b side's
    own pairs are band pairs of other buckets."""
    assert b0 >= base + 23
    reads = []
    quad = lambda r: (list(range(base + 4 * (r % 4), base + 4 * (r % 4) + 4)),
                      list(range(b0 + 4 * (r // 4), b0 + 4 * (r // 4) + 4)))
    for r in range(n // 16):
        a, b = quad(r)
        reads.append(a + b)
    rem = n % 16
    if rem:
        a, b = quad(n // 16)
        if rem // 4:
            reads.append(a + b[:rem // 4])
        if rem % 4:
            reads.append(a[:rem % 4] + [b[rem // 4]])
    return reads


def hash_reads_top(base, n, b0):
    return max(max(r) for r in hash_reads(base, n, b0))


def expect(overflow=(), pair_rerun=False, relabel=False):
    return types.SimpleNamespace(overflow_buckets=sorted(overflow), pair_rerun=pair_rerun, relabel=relabel)


def _filler(n_contigs, keep_out):
    """Filler contigs: every contig outside the buckets' ranges in keep_out."""
    ok = np.ones(n_contigs, bool)
    for lo, hi in keep_out:
        ok[max(lo, 0):hi] = False
    return np.flatnonzero(ok)


# ---- builders: (records, n_contigs, expect) -------------------------------------------
@functools.lru_cache(maxsize=None)
def build_pair_reduce_fill(n_hash, repeat=1, chunk=CHUNK):
    """n_contigs = 4096 (B = 256, one flush group, final_kernel<4096>): bucket 128
    gets exactly n_hash distinct hash pairs, each `repeat` times, no chunk above
    pcap = chunk / 8 pairs."""
    n, bucket = 4096, 128
    base = bucket << 4
    reads = hash_reads(base, n_hash, base + 24) * repeat
    top = hash_reads_top(base, n_hash, base + 24)
    rec = lay_out(spread(reads, chunk // 8), _filler(n, [(base - 3, top + 1)]), chunk)
    return rec, n, expect(overflow=[bucket] if n_hash > HASH_R_FILL else [])


MERGED_BUCKET = 16  # of 64: the middle buckets of 1,024 contigs have fewer than 8,193 pairs with b - a >= 8


@functools.lru_cache(maxsize=None)
def build_merged_groups(n_hash):
    """n_contigs = 1024 (B = 64, 4 flush groups, final_kernel<8192>): one bucket gets
    n_hash distinct hash pairs, none twice, evenly over the chunks, so every group
    stays below the pair reduce's limit and only the merge can overflow."""
    n, bucket = 1024, MERGED_BUCKET
    base = bucket << 4
    reads = hash_reads(base, n_hash, base + 24)
    top = hash_reads_top(base, n_hash, base + 24)
    assert top < n
    rec = lay_out(spread(reads, CHUNK // 8), _filler(n, [(base - 3, top + 1)]))
    return rec, n, expect(overflow=[bucket] if n_hash > HASH_F else [])


@functools.lru_cache(maxsize=None)
def build_merged_same_lists():
    """The same 2,000 pairs in every quarter of the chunks: four identical lists, a
    merged list of 2,000 keys with count 4."""
    n, bucket = 1024, MERGED_BUCKET
    base = bucket << 4
    reads = hash_reads(base, 2000, base + 24)
    top = hash_reads_top(base, 2000, base + 24)
    quarter = spread(reads, CHUNK // 8)
    rec = lay_out(quarter * 4, _filler(n, [(base - 3, top + 1)]))
    return rec, n, expect()


@functools.lru_cache(maxsize=None)
def build_merged_one_bucket():
    """n_contigs = 16 (B = 1, 256 flush groups): every pair of the 16 contigs, all
    pair lists in one flush, so 255 groups are empty (part_n = -1)."""
    n = 16
    reads = [[a, b] for a in range(16) for b in range(a, 16)]
    rec = lay_out([reads], [0])
    return rec, n, expect()


@functools.lru_cache(maxsize=None)
def build_band_small(n, bucket):
    """Reads (a, a + d) for every a of one bucket and d = 0..9, a + d < n_contigs:
    d <= 3 compact codes, 4..7 general reads into the band, 8 and 9 the hash."""
    base = bucket << 4
    reads = [[a, a + d] if d else [a] for a in range(base, min(base + 16, n)) for d in range(10) if a + d < n]
    rec = lay_out(spread(reads, CHUNK // 8), _filler(n, [(base - 3, base + 26)]))
    return rec, n, expect()


@functools.lru_cache(maxsize=None)
def build_band_full_wide():
    """n_contigs = 262,160 (bw = 10, B = 257): bucket 128 has all 8,192 band slots
    nonzero and 3,584 hash pairs: 11,776 output pairs of at most 16,384."""
    n, bucket = 262_160, 128
    base = bucket << 10
    reads = [[a, a + d] if d else [a] for a in range(base, base + 1024) for d in range(8)]
    reads = interleave(reads, hash_reads(base, HASH_R_FILL, base + 24))
    rec = lay_out(spread(reads, CHUNK // 8), _filler(n, [(base - 3, base + 1024 + 8)]))
    return rec, n, expect()


@functools.lru_cache(maxsize=None)
def build_compact_edges(n, overflowed):
    """Compact reads (every code M, spans 0..3) with m0 on and up to 3 below two
    bucket starts: bucket k's (also a code-bucket start) and bucket k + 1's (a
    pair-bucket start only); both receiving buckets clean, or both overflowed, so
    that bucket_widen_kernel regenerates the crossing pairs from the codes."""
    g = geometry(n)
    k = (g.B // 2) & ~3
    reads = []
    for start in (k << g.bw, (k + 1) << g.bw):
        for m0 in range(start - 3, start + 1):
            for M in range(8):
                r = [m0] + [m0 + i + 1 for i in range(3) if M >> i & 1]
                reads += [r[::-1] if M & 1 else r] * (1 + (m0 + M) % 3)
    keep = [((k << g.bw) - 6, ((k + 2) << g.bw))]
    if overflowed:
        wide = []
        for b in (k, k + 1):
            base = b << g.bw
            wide += hash_reads(base, HASH_R_FILL + 1, ((k + 2) << g.bw) + 32 + 256 * (b - k))
        keep.append((((k + 2) << g.bw) + 32, ((k + 2) << g.bw) + 32 + 512))
        reads = interleave(wide[::2] + wide[1::2], reads)
    rec = lay_out(spread(reads, CHUNK // 8), _filler(n, keep))
    return rec, n, expect(overflow=[k, k + 1] if overflowed else [])


LOOKBACK_TOP = 240  # bucket 255 of 4,096 contigs has 36 pairs with b - a >= 8: 240 is the last that can overflow


@functools.lru_cache(maxsize=None)
def build_lookback(gap):
    """n_contigs = 4096: every bucket holds a few pairs and buckets 0, 63, 64, 65,
    128 and 240 overflow (3,585 hash pairs each), so lookback_offset crosses more
    than 64 buckets with zero-length ones among them and assemble2_kernel places
    every list again.  gap: buckets 1..70 are empty instead (overflow: 0, 128,
    240).  The wide reads fill their chunks, so the pair lists are built twice."""
    n = 4096
    over = [0, 128, LOOKBACK_TOP] if gap else [0, 63, 64, 65, 128, LOOKBACK_TOP]
    reads, keep = [], []
    for b in over:
        base = b << 4
        b0 = max(base + 24, 71 * 16 + 8) if gap else base + 24
        reads += hash_reads(base, HASH_R_FILL + 1, b0)
    if gap:
        keep.append((16, 71 * 16))
        few = [c for c in range(0, n - 12, 16) if not 16 <= c < 71 * 16]
    else:
        few = list(range(0, n - 12, 16))
    reads += [[c + 2, c + 12] for c in few] + [[c + 5, c + 6] for c in few]
    rng = np.random.default_rng(13)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    per = -(-len(reads) // 8)
    rec = lay_out([reads[i:i + per] for i in range(0, len(reads), per)], _filler(n, keep))
    return rec, n, expect(overflow=over, pair_rerun=True)


@functools.lru_cache(maxsize=None)
def build_split_overflow(n):
    """An overflowed bucket, for split bounds inside it and inside the next one."""
    if n == 1024:
        return build_merged_groups(HASH_F + 1)
    return build_pair_reduce_fill(HASH_R_FILL + 1)


@functools.lru_cache(maxsize=None)
def build_split_big_read(n):
    """A clean list and one read of 9 records (the host merges it after the final kernel)."""
    g = geometry(n)
    base = (g.B // 2) << g.bw
    reads = hash_reads(base, 100, base + 24) + [[c, c + 9] for c in range(5, n - 20, 37)]
    reads.append([7 + 11 * i for i in range(9)])
    rec = lay_out(spread(reads, CHUNK // 8), np.arange(n))
    return rec, n, expect()


def _exact_pairs(total):
    """Reads of 2, 3 and 4 distinct wide contigs (3, 6, 10 pairs) with `total` pairs."""
    sizes = {0: [], 1: [4], 2: [4, 4]}[total % 3]  # 10 = 1 (mod 3)
    rest = total - 10 * len(sizes)
    sizes += [3] * min(4, rest // 6)
    rest = total - sum(u * (u + 1) // 2 for u in sizes)
    assert rest >= 0 and rest % 3 == 0
    sizes += [2] * (rest // 3)
    return sizes


@functools.lru_cache(maxsize=None)
def build_pair_capacity(extra, chunk=CHUNK):
    """Three chunks; the middle one's general reads give pcap + extra pairs."""
    n = 8192
    pcap = chunk // 8
    reads = [[100 + 40 * i + 9 * j for j in range(u)] for i, u in enumerate(_exact_pairs(pcap + extra))]
    rec = lay_out([[], reads, []], np.arange(n), chunk)
    return rec, n, expect(pair_rerun=extra > 0)


@functools.lru_cache(maxsize=None)
def build_second_attempt(suspect, chunk=CHUNK):
    """Three chunks, the middle one full of reads of 8 records on 8 contigs of their
    own, 4.5 pairs per record.  Aligned: chunk / 8 reads, chunk * 9 / 2 pairs.
    suspect: a read of 7 records at the chunk's records 0..6, then reads of 8
    whose last starts at the chunk's last record, so the chunk's reads cover
    chunk + 7 records: 28 + 36 * chunk / 8 pairs, 28 more than chunk * 9 / 2.
    All of these are wide: the relabelled rerun comes first and keeps them general."""
    n = 8192
    sizes = ([7] if suspect else []) + [8] * (chunk // 8)
    rows, rid, c = [], 0, 0
    for i in range(chunk):  # an ordinary chunk: compact reads of 1 and 2 records
        rows.append((rid, 5000 + (i // 2) % 1000 + (i & 1)))
        rid += (i & 1) or (i % 6 == 0)
    rid += 1
    for u in sizes:
        rows += [(rid, c + (j * 5) % u) for j in range(u)] if u == 8 else [(rid, c + j) for j in range(u)]
        rid, c = rid + 1, c + u
    while len(rows) < 3 * chunk:
        rows.append((rid, 6500 + rid % 1000))
        rid += 1
    rec = np.array(rows, np.uint32)
    return rec, n, expect(pair_rerun=True, relabel=True)


# every case of the GPU tests: name -> (builder, args, KARMA_CHUNK)
CASES = {
    "reduce_3583": (build_pair_reduce_fill, (3583,), None),
    "reduce_3584": (build_pair_reduce_fill, (3584,), None),
    "reduce_3585": (build_pair_reduce_fill, (3585,), None),
    "reduce_4096": (build_pair_reduce_fill, (4096,), None),
    "reduce_3584_x3": (build_pair_reduce_fill, (3584, 3), None),
    "reduce_3584_chunk2048": (build_pair_reduce_fill, (3584, 1, 2048), 2048),
    "merged_8191": (build_merged_groups, (8191,), None),
    "merged_8192": (build_merged_groups, (8192,), None),
    "merged_8193": (build_merged_groups, (8193,), None),
    "merged_same_lists": (build_merged_same_lists, (), None),
    "merged_one_bucket": (build_merged_one_bucket, (), None),
    "band_first": (build_band_small, (4096, 0), None),
    "band_last": (build_band_small, (4096, 255), None),
    "band_last_4090": (build_band_small, (4090, 255), None),
    "band_full_bw10": (build_band_full_wide, (), None),
    "compact_bw4_clean": (build_compact_edges, (4096, False), None),
    "compact_bw4_overflowed": (build_compact_edges, (4096, True), None),
    "compact_bw7_clean": (build_compact_edges, (20_000, False), None),
    "compact_bw7_overflowed": (build_compact_edges, (20_000, True), None),
    "compact_bw10_clean": (build_compact_edges, (262_160, False), None),
    "compact_bw10_overflowed": (build_compact_edges, (262_160, True), None),
    "lookback": (build_lookback, (False,), None),
    "lookback_gap": (build_lookback, (True,), None),
    "pcap": (build_pair_capacity, (0,), None),
    "pcap_plus_1": (build_pair_capacity, (1,), None),
    "pcap_chunk2048": (build_pair_capacity, (0, 2048), 2048),
    "pcap_plus_1_chunk2048": (build_pair_capacity, (1, 2048), 2048),
    "second_attempt_exact": (build_second_attempt, (False,), None),
    "second_attempt_suspect": (build_second_attempt, (True,), None),
    "second_attempt_suspect_chunk2048": (build_second_attempt, (True, 2048), 2048),
}


def case(name):
    builder, args, chunk = CASES[name]
    return builder(*args) + (chunk,)


@functools.lru_cache(maxsize=None)
def case_model(name):
    rec, n, _, _ = case(name)
    return pair_graph(rec, n)
