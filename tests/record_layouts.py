"""Record layouts shared by the GPU tests (no test in here)."""
import numpy as np

CHUNK_EDGE = 4096  # every multiple is an edge of classify's chunks: chunk_records returns 4,096 or 8,192


def chunk_edge_records(n=3000, total=40_000, seed=29, wide_edge=None):
    """(read, contig) records, grouped by read: compact reads of 1..4 records
    (contigs lo + 0..3), and at every multiple of 4,096 records one compact
    read of m in {9, 12, 16} records that (a) ends exactly at the edge, (b)
    straddles it with 1..7 records past it, or (c) starts exactly at it --
    every (m, position) once over the 9 edges below 40,000.  With flagged
    records (16 per lane) such a read is a code inside a chunk; classify's
    chunk-end tail walk must treat it alike.  wide_edge = i: the read at edge i
    spreads over 200 contig ids instead (general and longer than 8 records: a
    big read, the positive control).  Returns (records, [(start, m, position)])."""
    rng = np.random.default_rng(seed)
    rows, placed = [], []
    r = 0

    def read(m, wide=False):
        nonlocal r
        lo = int(rng.integers(0, n - 200))
        cs = lo + (rng.integers(0, 200, m) if wide else rng.integers(0, 4, m))
        rows.extend((r, int(c)) for c in cs)
        r += 1

    def fill(to):
        while len(rows) < to:
            read(min(int(rng.integers(1, 5)), to - len(rows)))

    combos = [(m, pos) for m in (9, 12, 16) for pos in "abc"]
    for i, edge in enumerate(range(CHUNK_EDGE, total, CHUNK_EDGE)):
        m, pos = combos[i % len(combos)]
        past = {"a": 0, "b": int(rng.integers(1, 8)), "c": m}[pos]  # the read's records at or past the edge
        fill(edge - (m - past))
        placed.append((len(rows), m, pos))
        read(m, wide=i == wide_edge)
    fill(total)
    return np.array(rows, np.uint32), placed
