"""The binned classify's LDS layout (graph_sets.hip classify2_kernel): bucket
queues sized by the job's code buckets (dynamic LDS), the quarter-size
transpose / staging buffer of the flagged walk (four transpose passes of 16
lanes, 256 staged codes, bin_stage after every four emit points) and the
occupancy they buy.  Every graph is bit-exact against the oracle, in both
record formats, with 4,096- and 8,192-record chunks.

Code buckets hold 2^bwc contigs with bwc = 6 up to 4,096 contigs and 12 at
config 3's size (make_geo), so Bc = 1, 49, 56, 57 are n_contigs = 64, 3,136
(and 200,000), 3,584 (and 229,376) and 3,648."""

import ctypes

import numpy as np
import pytest

from karma_amd import _lib, engine
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["4096", "8192"])
def chunk(request, monkeypatch):
    monkeypatch.setenv("KARMA_CHUNK", request.param)
    return int(request.param)


def check(rec, n):
    """Both record formats against the oracle's graph, bit for bit."""
    rec = np.asarray(rec, np.uint32)
    r = rec.astype(np.int64)
    starts = np.flatnonzero(np.r_[True, r[1:, 0] != r[:-1, 0]])
    o = oracle.graph_groups(np.r_[starts, len(r)], r[:, 1], None, None, n, dedup=True)
    for x in (engine.graph_from_records(rec, n), engine.graph_from_records(engine.flag_records(rec), n, flagged=True)):
        assert np.array_equal(x.a, o["a"])
        assert np.array_equal(x.b, o["b"])
        assert np.array_equal(x.shared, o["shared"])
        assert np.array_equal(x.weight.view(np.uint64), o["weight"].view(np.uint64))
        assert np.array_equal(x.totals, o["totals"])


def fails(rec, n):
    rec = np.asarray(rec, np.uint32)
    for flagged in (False, True):
        with pytest.raises(_lib.KarmaError):
            engine.graph_from_records(engine.flag_records(rec) if flagged else rec, n, flagged=flagged)


class Rows:
    """(read, contig) records appended read by read."""

    def __init__(self, seed, n):
        self.rng = np.random.default_rng(seed)
        self.n = n
        self.rows = []
        self.r = 0

    def __len__(self):
        return len(self.rows)

    def read(self, contigs):
        self.rows.extend((self.r, int(c)) for c in contigs)
        self.r += 1

    def compact(self, m, lo=None, hi=None):
        """A read of m records whose contigs lie in [m0, m0 + 3], m0 in [lo, hi)."""
        lo = 0 if lo is None else lo
        hi = max(lo + 1, self.n - 3) if hi is None else hi
        m0 = int(self.rng.integers(lo, hi))
        self.read(np.minimum(m0 + self.rng.integers(0, 4, m), self.n - 1) if m > 1 else [m0])

    def wide(self, m):
        """A general read: contigs spread over more than 4 ids."""
        lo = int(self.rng.integers(0, max(1, self.n - 60)))
        self.read([lo, min(self.n - 1, lo + 40)] + list(np.minimum(lo + self.rng.integers(0, 50, max(0, m - 2)),
                                                                   self.n - 1)))

    def fill_to(self, k, m=(1, 4)):
        """Short compact reads over every bucket until exactly k records."""
        while len(self) < k:
            self.compact(min(k - len(self), int(self.rng.integers(*m))))

    def array(self):
        return np.array(self.rows, np.uint32)


@pytest.mark.parametrize("n", [64, 3136, 3584, 3648, 200_000, 229_376])
def test_bucket_counts(n, chunk):
    """Bc = 1, 49, 56 (binned; the queues are the launch's dynamic LDS) and 57
    (the partition path), reads spread so that every queue of a chunk is used."""
    t = Rows(n, n)
    t.fill_to(40_000)
    check(t.array(), n)


def test_one_bucket_overflows(chunk):
    """One chunk in which a single bucket receives more than 64 and more than
    128 codes (back segments; a queue refilled behind its flush), the other
    buckets a few each."""
    n = 3136
    t = Rows(7, n)
    t.fill_to(1000)
    for i in range(150):  # bucket 7 (contigs 448 .. 511): 150 codes in a row, then interleaved
        t.compact(1, 448, 509)
    for i in range(100):
        t.compact(2, 448, 509)
        t.compact(1)
    t.fill_to(20_000)
    check(t.array(), n)


@pytest.mark.parametrize("k", [1, 7, 8, 9, 63, 64, 65])
def test_exact_fills(k, chunk):
    """Every chunk gives bucket 5 exactly k codes (the padding of its last
    16-byte granule, a queue that fills exactly, one code past a flush)."""
    n = 3136
    t = Rows(100 + k, n)
    for c in range(4):
        end = (c + 1) * chunk
        for i in range(k):
            t.compact(1, 320, 381)  # bucket 5: contigs 320 .. 383
        while len(t) < end:  # the rest: reads of the buckets above it, none across the chunk's end
            t.compact(min(end - len(t), int(t.rng.integers(1, 4))), 384, n - 3)
    check(t.array(), n)


@pytest.mark.parametrize("n", [3136, 200_000])
def test_staging_capacity(n, chunk):
    """Full steps in which every record is its own read (1,024 codes per step
    of flagged records, 64 at every emit point: the staging buffer is drained
    after every four), then long reads, from a chunk's start and from a step
    in its middle."""
    t = Rows(31, n)
    for _ in range(3 * 1024 + 300):
        t.compact(1)
    for _ in range(40):
        t.compact(16)
    for _ in range(20):
        t.compact(int(t.rng.integers(17, 41)))
    t.fill_to(2 * 8192 + 1024)
    for _ in range(4 * 1024):
        t.compact(1)
    for _ in range(30):
        t.compact(int(t.rng.integers(9, 17)))
        t.wide(int(t.rng.integers(9, 30)))
    t.fill_to(30_000)
    check(t.array(), n)


@pytest.mark.parametrize("res", [0, 1, 63])
def test_chunk_code_counts_mod_64(res, chunk):
    """Chunks whose code count is = 0, 1 and 63 (mod 64): the last batch of
    staged codes of a chunk is full, one code, one short of full."""
    n = 3136
    t = Rows(200 + res, n)
    for c in range(3):
        codes = (chunk // 2 // 64 + 8) * 64 + res  # one- and two-record reads: codes in [chunk / 2, chunk]
        twos, ones = chunk - codes, 2 * codes - chunk
        kinds = np.r_[np.ones(ones, int), np.full(twos, 2)]
        t.rng.shuffle(kinds)
        for m in kinds:
            t.compact(int(m))
        assert len(t) == (c + 1) * chunk
    check(t.array(), n)


def test_rare_step_after_a_remainder(chunk):
    """A step with general and big reads (replayed after the chunk's loop)
    directly after steps whose staged codes are no multiple of 64."""
    n = 3136
    t = Rows(41, n)
    for c in range(3):
        base = c * chunk
        for _ in range(333):  # 333 codes in the first step(s)
            t.compact(1)
        t.fill_to(base + 1024 + 5, (2, 3))
        t.wide(6)
        t.wide(12)
        t.compact(13)
        t.fill_to(base + 2048 + 3, (1, 3))
        t.wide(3)
        t.fill_to(base + chunk)
    check(t.array(), n)


@pytest.mark.parametrize("pos", [1022, 1023, 4094, 8190, 8191])
def test_range_error_of_a_code_at_a_step_boundary(pos, chunk):
    """A compact read with a contig >= N that ends a step, straddles into the
    next one or ends a chunk, behind a number of codes that is no multiple of
    64: the call fails with the range error; the same read below N matches."""
    n = 3136
    for bad in (True, False):
        t = Rows(pos, n)
        t.fill_to(pos, (1, 2))
        top = n if bad else n - 1
        t.read([n - 2, top])
        t.fill_to(20_000)
        (fails if bad else check)(t.array(), n)


@pytest.mark.parametrize("pos", [127, 255, 383, 511, 767, 1023, 4095, 8191])
def test_reads_across_transpose_passes(pos, chunk):
    """Reads of 2, 3 and 12 records that straddle the lanes 15/16, 31/32 and
    47/48 of a step (records 256, 512, 768 of a flagged step; 128, 256, 384 of
    a pairs step), lane 63 into the next step and the chunk's end, near N (the
    construction of test_gpu_parity.test_records_contig_range_per_read_kind):
    every contig < N matches the oracle, one >= N fails the call."""
    n = 3136
    for read in ([n - 2, n - 1], [n - 4, n - 1, n - 2], [5, 900, n - 1], [10 + i for i in range(11)] + [n - 1]):
        t = Rows(pos + len(read), n)
        t.fill_to(8192 + pos, (1, 2))
        t.read(read)
        t.fill_to(8192 + pos + 12_000)
        check(t.array(), n)
    for read in ([n - 2, n], [n - 1, n + 2, n - 1], [5, 900, n + 7]):
        t = Rows(pos + len(read), n)
        t.fill_to(8192 + pos, (1, 2))
        t.read(read)
        t.fill_to(8192 + pos + 12_000)
        fails(t.array(), n)


def test_occupancy():
    """The LDS diet's occupancy, from the occupancy query with the job's
    dynamic LDS: 5 blocks per CU for config 3's 200,000 contigs (49 code
    buckets) on flagged records, at least 4 at 229,376 (56) and on pairs."""
    ctx = _lib.default_context()

    def blocks(n, fmt):
        out = ctypes.c_int(0)
        _lib.call("karma_graph_classify_occupancy", ctx.h, n, fmt, ctypes.byref(out))
        return out.value

    assert blocks(200_000, _lib.KARMA_REC_FLAGGED) == 5
    assert blocks(229_376, _lib.KARMA_REC_FLAGGED) >= 4
    assert blocks(200_000, _lib.KARMA_REC_SORTED) >= 4
    assert blocks(229_377, _lib.KARMA_REC_FLAGGED) >= 4  # 57 code buckets: the unbinned classify
