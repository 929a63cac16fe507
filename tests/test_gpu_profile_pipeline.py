"""The wave-per-contig profile's contig loop (kmer.hip profile_wave_kernel)
against the oracle.

A wave loads the next contig's offsets while it counts the current one and the
next contig's first 1,024-position stage of packed words before it writes the
current row; later stages load inside the counting, and contigs with exception
bases stage their mask words too.  The cases here sit on the stage boundaries
(1,024 and 2,048 positions), give a wave no, one or two rows and a next contig
that does not exist, put exception contigs next to clean ones, end the store
inside the words a stage reads, and take the u16 and the u32 counters.
Everything is bit-exact against oracle.calc_kmer_profile.
"""
from collections import OrderedDict

import numpy as np
import pytest

from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import ShardedBuild
from oracle import oracle

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


def lengths_for(kmin):
    # kmin - 1: no k-mer (an all-zero row); 1,024 positions end a stage at
    # L = 1,023 + kmin, 2,048 at L = 2,047 + kmin (5p6: 1,028 and 2,052)
    return [5, 6, kmin - 1, 1027, 1028, 1029, 1030, 2052, 2053, 3100, 1022 + kmin, 1023 + kmin, 1024 + kmin,
            2047 + kmin, 2048 + kmin]


def make_seqs(lengths, seed, exc=()):
    """Random ACGT contigs of the given lengths; those listed in `exc` get a few N."""
    rng = np.random.default_rng(seed)
    seqs = OrderedDict()
    for i, L in enumerate(lengths):
        b = ACGT[rng.integers(0, 4, L)].copy()
        if i in exc and L:
            b[rng.integers(0, L, 1 + L // 300)] = ord("N")
        seqs[f">ctg{i}"] = b.tobytes().decode()
    return seqs


def oracle_profile(seqs, kmer):
    """The oracle's profile, columns and row totals.  A contig shorter than
    the smallest k has no k-mer: its row is all zero and adds no column.  The
    reference ends the run over such a row (kmer.py:250-258, and so does the
    oracle), so the oracle gets the other contigs and the short ones' rows
    must come back as zeros."""
    kmin = 5 if kmer == "5p6" else kmer
    keep = [i for i, v in enumerate(seqs.values()) if len(v) >= kmin]
    sub = OrderedDict((k, v) for k, v in seqs.items() if len(v) >= kmin)
    oprof, ocols, ocounts = oracle.calc_kmer_profile(sub, kmer)
    prof = np.zeros((len(seqs), oprof.shape[1]), np.float64)
    tot = np.zeros(len(seqs), np.int64)
    prof[keep] = oprof
    tot[keep] = ocounts.sum(axis=1)
    return prof, ocols, tot


def check(seqs, kmer):
    prof, cols, tot = engine.kmer_profile(seqs, kmer)
    oprof, ocols, otot = oracle_profile(seqs, kmer)
    assert cols == ocols
    assert prof.shape == oprof.shape
    assert np.array_equal(prof.view(np.uint64), oprof.view(np.uint64))
    assert np.array_equal(tot, otot)


@pytest.mark.parametrize("kmer", ["5p6", 4])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 45])
def test_stage_boundary_lengths(kmer, n):
    """Every length beside every other as the next contig (three shuffles of
    the list), and the first n of them alone: with 8 waves per block, 7, 8 and
    9 contigs leave a wave of the first block without a row or give the second
    block one row."""
    base = lengths_for(5 if kmer == "5p6" else kmer)
    rng = np.random.default_rng(11)
    lengths = base + [base[i] for i in rng.permutation(len(base))] + [base[i] for i in rng.permutation(len(base))]
    check(make_seqs(lengths[:n], 12), kmer)


@pytest.mark.parametrize("n", [6143, 6144, 6145, 12289])
def test_rows_per_wave_around_the_launch(n):
    """6,144 waves are resident on 256 CUs (3 blocks of 8 waves each): waves
    with no, one, two and three rows, the look-ahead running past n; every
    40th contig reaches a second or third stage."""
    rng = np.random.default_rng(n)
    lengths = rng.integers(4, 40, n)
    lengths[::40] = rng.choice([1028, 1029, 2052, 2053, 2500], len(lengths[::40]))
    check(make_seqs(lengths.tolist(), n + 1), "5p6")


@pytest.mark.parametrize("kmer", ["5p6", 4])
def test_exception_contigs_beside_clean_ones(kmer):
    """Contigs with exception bases stage their mask words beside the packed
    ones: clean -> exception -> clean at every stage count, in
    one wave's sequence (a single block: consecutive rows of a wave are 8
    apart) and across many blocks."""
    base = [30, 1029, 2053, 3100, 6, 1028]
    for reps, exc_every in ((4, 2), (4, 3), (400, 7)):
        lengths = base * reps
        exc = {i for i in range(len(lengths)) if (i // 8) % exc_every == 1 or i % 11 == 3}
        check(make_seqs(lengths, 21 + reps, exc), kmer)


@pytest.mark.parametrize("last", [4, 5, 1029, 2053])
def test_store_ends_inside_a_stage_read(last):
    """The store's last contig ends within the 65 words a stage load reads (the
    zero words past the store cover it), as the only contig and behind others."""
    if last >= 5:
        check(make_seqs([last], 31), "5p6")
    check(make_seqs([700, 1029, 33] * 5 + [last], 32), "5p6")


def test_u32_counters_with_a_long_contig():
    """One contig of 65,536 bases or more switches the launch to u32 counters;
    the long contig itself runs 64 stages."""
    lengths = lengths_for(5)
    for at in (0, 7, len(lengths)):
        ls = lengths[:at] + [70_000] + lengths[at:]
        check(make_seqs(ls, 41 + at, exc={3}), "5p6")
    check(make_seqs(lengths[:6] + [65_536], 44), 4)


def test_same_store_profiled_twice():
    seqs = make_seqs(lengths_for(5) * 3, 51, exc={4, 20})
    oprof, _, _ = oracle_profile(seqs, "5p6")
    ctx = _lib.default_context()
    store = engine.ContigStore(ctx, *engine.encode_sequences(seqs))
    plan = engine.KmerPlan(ctx, store, engine.kmode_of("5p6"))
    try:
        plan.finalize()
        first = plan.profile_host().copy()
        second = plan.profile_host()
        assert np.array_equal(first.view(np.uint64), oprof.view(np.uint64))
        assert np.array_equal(second.view(np.uint64), oprof.view(np.uint64))
    finally:
        plan.close()
        store.close()


@pytest.mark.parametrize("flagged", [False, True])
def test_deferred_step_profile_reads_m_on_the_device(flagged):
    lengths = lengths_for(5) * 2 + [30] * 70
    n = len(lengths)
    seqs = make_seqs(lengths, 61, exc={2, 9, 40})
    oprof, ocols, _ = oracle_profile(seqs, "5p6")
    rec = np.ascontiguousarray(engine.synth_records(61, n, 0, 20_000, True))
    ctx = _lib.Context(0)
    build = ShardedBuild(ctx, SoloComm(), -1, n, 0, n, flagged=flagged)
    store = engine.ContigStore(ctx, *engine.encode_sequences(seqs))
    dev = _lib.DevBuf.from_numpy(ctx, engine.flag_records(rec) if flagged else rec.view(np.int64).reshape(-1))
    try:
        assert build.native is not None
        for _ in range(2):
            assert build.run(store, dev.ptr, len(rec), count=False)["E_local"] is None
        build.sync()
        got = build.native.profile().numpy()
        assert got.shape == oprof.shape
        assert np.array_equal(got.view(np.uint64), oprof.view(np.uint64))
        res = build.run(store, dev.ptr, len(rec), keep=True)
        assert engine.decode_keys(res["columns"], -1) == ocols
        assert np.array_equal(res["profile"].numpy().view(np.uint64), oprof.view(np.uint64))
    finally:
        build.close()
        store.close()
        dev.close()
        ctx.close()
