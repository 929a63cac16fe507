"""The binned code reduce (graph_sets.hip code_seg_reduce_kernel) against the oracle.

With at most 56 code buckets the classify writes every wave chunk's compact
codes as per-bucket segments, and one reduce block per (bucket, group of
chunks) counts them: the chunk's front slot (or its packed front granules),
then the back segments of the chunks whose queue filled.  A wave takes a
batch of 64 chunks of every 1,024 of its group.  On slotted fronts it streams
batches without guards while its current batch and its next two lie wholly
inside the group (from 2,112 chunks per group on for wave 0, 64 more for each
further wave) and the group's last batches with guards.  The cases put the
chunk count on both sides of a batch (64) and of a block's round (1,024), in
both front layouts, with one and with several groups per bucket, and, in
groups of 2,111 to 4,160 chunks, on both sides of a wave's entering the
unguarded loop, of its second round there, and of its hand-over to the guarded
batches, with back segments listed and the list overflowing.  Everything is
bit-exact against
oracle.graph_groups, through karma_graph_records (pairs and flagged records)
and through a deferred step followed by a kept step.
"""
import numpy as np
import pytest

from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import ShardedBuild
from oracle import oracle

pytestmark = pytest.mark.gpu

CHUNK = 2048  # records per classify chunk (the smallest KARMA_CHUNK takes)


def rows_of(m0, M):
    """(read, contig) rows of compact reads: read i hits contig m0[i] and
    contig m0[i] + 1 + j for every set bit j of M[i] (its code is
    m0_local << 3 | M in the code bucket of m0)."""
    m0 = np.asarray(m0, np.int64)
    M = np.asarray(M, np.int64)
    hit = np.concatenate([np.ones((len(m0), 1), bool), ((M[:, None] >> np.arange(3)) & 1).astype(bool)], 1)
    contig = m0[:, None] + np.arange(4)
    read = np.broadcast_to(np.arange(len(m0))[:, None], hit.shape)
    return np.ascontiguousarray(np.stack([read[hit], contig[hit]], 1).astype(np.uint32))


def random_rows(seed, n, A):
    """A records of random compact reads over n contigs (the last read may be cut)."""
    rng = np.random.default_rng(seed)
    R = A if A < 1 << 20 else A // 2  # a read has at least one record, 2.5 on average
    m0 = rng.integers(0, max(1, n - 3), R)
    M = rng.integers(0, 8, R) if n > 3 else np.zeros(R, np.int64)
    return rows_of(m0, M)[:A]


def oracle_graph(rec, n):
    rs = np.asarray(rec, np.int64)
    st = np.flatnonzero(np.r_[True, rs[1:, 0] != rs[:-1, 0]])
    return oracle.graph_groups(np.r_[st, len(rs)], rs[:, 1], None, None, n, dedup=True)


def same(e, o):
    assert np.array_equal(e.a, o["a"]) and np.array_equal(e.b, o["b"])
    assert np.array_equal(e.shared, o["shared"])
    assert np.array_equal(e.weight.view(np.uint64), o["weight"].view(np.uint64))
    assert np.array_equal(e.totals, o["totals"])


def check_records(rec, n, o=None):
    o = oracle_graph(rec, n) if o is None else o
    same(engine.graph_from_records(rec, n, grouped=True), o)
    same(engine.graph_from_records(engine.flag_records(rec), n, flagged=True), o)
    return o


# n contigs -> code buckets of 64 contigs (Bc = n / 64); at 2,048-record chunks
# the fronts are whole slots up to 17 buckets and packed granules from 18 on;
# a bucket gets one group per 2^19 records it may hold (256 chunks), so one
# bucket (n = 64) has 1, 2, 4 and 5 groups below and 8 or 20 buckets have one.
# 333 and 1,023 chunks are no multiple of their 2 and 4 groups.
@pytest.mark.parametrize("n,chunks", [(64, 1), (64, 63), (64, 64), (64, 65), (64, 333), (64, 1023), (64, 1025),
                                      (512, 65), (512, 1025), (1280, 1), (1280, 65), (1280, 1025)])
@pytest.mark.parametrize("cut", [0, 700])  # the last chunk whole / partly filled
def test_chunk_counts_groups_and_front_layouts(n, chunks, cut, monkeypatch):
    monkeypatch.setenv("KARMA_CHUNK", str(CHUNK))
    check_records(random_rows(7 * chunks + n + cut, n, chunks * CHUNK - cut), n)


# The unguarded loop.  1,088 contigs are 17 code buckets, the most that keep
# slotted fronts at 2,048-record chunks, and one group up to 17 * 2^19 records
# (4,352 chunks).  Wave w starts at chunk 64 w of its group and streams
# unguarded while c0 + 2,112 <= the group's chunks, two batches a round:
#   2,111  no wave enters;            2,112 / 2,113  wave 0 alone (one round);
#   3,135  every wave, one round (the last needs 15 * 64 + 2,112 = 3,072);
#   3,136  the same, the guarded batches one chunk longer;
#   4,159 / 4,160  wave 0 on either side of its second round (2,048 + 2,112).
# After its last round a wave's current set was loaded unguarded and is
# counted by the guarded loop.  5,000 chunks are two groups of 2,500.
@pytest.mark.parametrize("chunks,cut", [(2111, 0), (2112, 0), (2112, 700), (2113, 0), (3135, 700), (3136, 0),
                                        (4159, 0), (4160, 0), (4160, 700), (5000, 700)])
def test_unguarded_batches_of_a_long_group(chunks, cut, monkeypatch):
    monkeypatch.setenv("KARMA_CHUNK", str(CHUNK))
    check_records(random_rows(chunks + cut, 1088, chunks * CHUNK - cut), 1088)


@pytest.mark.parametrize("heavy_every", [2, 1])
def test_back_segments_listed_from_unguarded_batches(heavy_every, monkeypatch):
    """2,300 chunks in one group of 17 buckets, reads of one record (record i
    is read i, in chunk i // CHUNK).  A heavy chunk puts a quarter of its
    reads into bucket 5 (~500 codes: 7 back segments), another a hundredth
    (~20 codes: none); the other buckets share the rest (~100 codes a chunk:
    one back segment each).  Every second chunk heavy: bucket 5's block lists
    ~1,150 chunks from its unguarded batches; every chunk heavy: 2,300, past
    the list's 2,048, so that block scans all chunks (the other buckets'
    blocks list all 2,300 either way)."""
    monkeypatch.setenv("KARMA_CHUNK", str(CHUNK))
    rng = np.random.default_rng(heavy_every)
    A = 2300 * CHUNK - 77
    pos = np.arange(A)
    share = np.where((pos // CHUNK) % heavy_every == 0, 0.25, 0.01)
    other = rng.integers(0, 1085 - 64, A)
    other += np.where(other >= 320, 64, 0)  # not in bucket 5 (contigs 320..383)
    m0 = np.where(rng.random(A) < share, rng.integers(320, 384, A), other)
    check_records(rows_of(m0, np.zeros(A, np.int64)), 1088)


def hand_built(n_chunks=40):
    """192 contigs = 3 code buckets.  Almost every read is one record in bucket
    0, so each 2,048-record chunk fills bucket 0's 64-code queue about 30
    times (as many back segments: directory bytes past the header's 16 are
    read); bucket 1 holds no read;
    bucket 2 and the corners of bucket 0 get single reads: m0_local 0 and 63
    (a bucket's last contig), M 0 and 7.  The last chunk is partly filled."""
    rng = np.random.default_rng(5)
    A = n_chunks * CHUNK - 300
    m0 = rng.integers(0, 61, A)
    M = np.zeros(A, np.int64)
    corners = [(0, 0), (0, 7), (63, 0), (63, 7), (128, 0), (128, 7), (191, 0), (188, 7), (60, 7)]
    at = rng.choice(A - 64, 40 * len(corners), replace=False)
    for i, p in enumerate(at):
        m0[p], M[p] = corners[i % len(corners)]
    return rows_of(m0, M)[:A], 192


@pytest.fixture(scope="module")
def hand():
    rec, n = hand_built()
    return rec, n, oracle_graph(rec, n)


@pytest.mark.parametrize("backlist", [None, "3", "0"])  # the block's list of chunks with back segments overflows
def test_back_segments_directory_and_list_overflow(hand, backlist, monkeypatch):
    rec, n, o = hand
    monkeypatch.setenv("KARMA_CHUNK", str(CHUNK))
    if backlist is not None:
        monkeypatch.setenv("KARMA_BACKLIST", backlist)
    check_records(rec, n, o)


def test_back_segments_in_some_chunks_only(monkeypatch):
    """Two buckets; bucket 1's queue fills (more than 64 codes) in every third
    chunk only, bucket 0's in all of them: the back list holds some chunks."""
    monkeypatch.setenv("KARMA_CHUNK", str(CHUNK))
    rng = np.random.default_rng(6)
    A = 90 * CHUNK - 11
    # reads of one record, so record i is read i and lies in chunk i // CHUNK:
    # a tenth of every third chunk's reads in bucket 1 (~205 codes), a
    # hundredth of the other chunks' (~20 codes, no back segment)
    pos = np.arange(A)
    share = np.where((pos // CHUNK) % 3 == 0, 0.1, 0.01)
    m0 = np.where(rng.random(A) < share, rng.integers(64, 128, A), rng.integers(0, 64, A))
    check_records(rows_of(m0, np.zeros(A, np.int64)), 128)


@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("case", ["hand", "groups"])
def test_deferred_step_then_kept_step(hand, case, flagged, monkeypatch):
    monkeypatch.setenv("KARMA_CHUNK", str(CHUNK))
    if case == "hand":
        rec, n, o = hand
    else:
        n = 64
        rec = random_rows(3, n, 333 * CHUNK - 5)  # one bucket, two groups
        o = oracle_graph(rec, n)
    ctx = _lib.Context(0)
    blob, offs, key_len = engine.synth_contigs(41, n, 30, 900, 0)
    build = ShardedBuild(ctx, SoloComm(), -1, n, 0, n, flagged=flagged)
    store = engine.ContigStore(ctx, blob, offs, key_len)
    dev = _lib.DevBuf.from_numpy(ctx, engine.flag_records(rec) if flagged else rec.view(np.int64).reshape(-1))
    try:
        assert build.native is not None
        assert build.run(store, dev.ptr, len(rec), count=False)["E_local"] is None
        build.sync()
        e_def, deferred = build.native.newest_edges()
        assert deferred
        same(e_def, o)
        res = build.run(store, dev.ptr, len(rec), keep=True)
        same(res["edges"], o)
    finally:
        build.close()
        store.close()
        dev.close()
        ctx.close()
