"""tests/kmer_reference.py against the oracle and against itself.  No GPU.

The model is what tests/test_gpu_kmer_stages.py holds the kernels to, so it is
pinned here first: bit-equal profile, equal columns and equal row totals with
oracle.c on a seeded alphabet soup for every k, and on every builder's input
where the dense arrays fit; pack() against a byte-by-byte loop; key_of() order
against Python str order; and each builder's claim counted from the model.
"""
import ctypes
import itertools
import random

import numpy as np
import pytest

import kmer_reference as kr
from oracle import oracle

ALPHABET = "ACGTACGTACGTNacgtRY\r-*\x00\xff"


def oracle_profile(seqs, kmer, key_lens):
    """oracle.calc_kmer_profile without its all-zero row and column exits, on explicit key lengths."""
    d = {str(i): s for i, s in enumerate(seqs)}
    blob, offs, _ = oracle.pack_sequences(d)
    raw, M = oracle.kmer_columns(d, kmer)
    N = len(seqs)
    prof, counts = np.zeros((N, M), np.float64), np.zeros((N, M), np.int64)
    kl = np.ascontiguousarray(key_lens, np.int64)
    rc = oracle.lib().oracle_kmer_profile(
        oracle._p(blob, ctypes.c_void_p), oracle._p(offs, oracle._i64p), oracle._p(kl, oracle._i64p), N,
        oracle.kmode_of(kmer), oracle._p(raw, ctypes.c_void_p), M, oracle._p(prof, oracle._f64p),
        oracle._p(counts, ctypes.c_void_p))
    assert rc == 0
    return prof, oracle.decode_keys(raw, M), counts.sum(axis=1)


def agree(seqs, kmer):
    kl = kr.key_lens(len(seqs))
    prof, cols, tot = oracle_profile(seqs, kmer, kl)
    mcols = kr.columns(seqs, kmer)
    assert mcols == cols
    assert np.array_equal(kr.row_totals(seqs, kmer), tot)
    assert np.array_equal(kr.profile(seqs, kmer, kl, mcols).view(np.uint64), prof.view(np.uint64))
    # the exchange points compose to the same columns
    km = kr.kmode_of(kmer)
    keys = kr.columns_of(kr.presence_bits(seqs, kmer), kr.exception_keys(seqs, kmer), kmer)
    assert [kr.kmer_of_key(x, km) for x in keys.tolist()] == cols


@pytest.mark.parametrize("kmer", [1, 2, 3, 5, 6, 7, 8, "5p6"])
def test_model_matches_oracle_on_alphabet_soup(kmer):
    rng = random.Random(100 + kr.kmin_of(kmer))
    k = kr.kmin_of(kmer)
    seqs = ["".join(rng.choice(ALPHABET) for _ in range(k + rng.randrange(0, 90))) for _ in range(220)]
    seqs[3] = seqs[3][:k]
    assert len(seqs) >= 200 and min(len(s) for s in seqs) >= k
    agree(seqs, kmer)


def test_built_in_constants_are_the_librarys():
    from karma_amd import _lib

    assert vars(_lib.kmer_tile()) == vars(kr.DEFAULTS)
    assert kr.T.STAGE_WORDS == kr.T.STAGE // 16 + 1 <= kr.T.PAD_WORDS and kr.T.LDS_COLS * 4 == 144 * 1024


def test_palindromes_of_exception_bytes_follow_str_semantics():
    seqs = ["N\0\0\0\0N", "\0ACCA\0", "nACCAn", "\0" * 7, "ACGTAN", "AACCAA", "NACCAn"]
    cols = kr.columns(seqs, "5p6")
    for t in ("N\0\0\0\0N", "\0ACCA\0", "nACCAn", "\0" * 6, "AACCAA"):
        assert t in cols and oracle.is_palindrome(t)
    assert "ACGTAN" not in cols and "NACCAn" not in cols
    agree(seqs, "5p6")


def test_pack_is_the_byte_loop():
    for lead, byte in [(0, ord("N")), (1, 0x00), (2, 0x80), (3, 0xFF)]:
        c = kr.store_case(lead, byte, lengths=tuple(range(41)) + (63, 64, 65))
        blob, offs, _ = kr.encode(c.seqs)
        packed, mask, woff, has_exc, nexc = kr.pack(blob, offs)
        w = 0
        total = 0
        for i, s in enumerate(c.seqs):
            assert woff[i] == w
            words = [0] * ((len(s) + 15) // 16)
            masks = [0] * len(words)
            bad = 0
            for j, ch in enumerate(s):
                if ch in "ACGT":
                    words[j // 16] |= "ACGT".index(ch) << (30 - 2 * (j % 16))
                else:
                    masks[j // 16] |= 1 << (15 - j % 16)
                    bad += 1
            assert packed[w:w + len(words)].tolist() == words and mask[w:w + len(words)].tolist() == masks
            assert has_exc[i] == (bad > 0)
            total += bad
            w += len(words)
        assert woff[-1] == w == len(packed) and nexc == total


def test_key_order_is_str_order():
    mixed = ["AAAAA", "AAAAAA", "AAAAC", "TTTTT", "TTTTTT", "\0\0\0\0\0", "\0\0\0\0\0\0", "N\0\0\0\0N", "N\0\0\0\0",
             "AAAA\0", "AAAA\xff", "\xff\xff\xff\xff\xff", "ACGGC", "ACGGCA", "ACGG\r", "nACCA", "nACCAn", "AAAAB"]
    for a, b in itertools.combinations(mixed, 2):
        assert (a < b) == (kr.key_of(a, -1) < kr.key_of(b, -1)), (a, b)
    for t in mixed:
        assert kr.kmer_of_key(kr.key_of(t, -1), -1) == t
    eight = ["AAAAAAAA", "AAAAAAAC", "\0AAAAAAA", "TTTTTTT\xff", "TTTTTTTT", "NNNNNNNN"]
    for a, b in itertools.combinations(eight, 2):
        assert (a < b) == (kr.key_of(a, 8) < kr.key_of(b, 8))
    # ordinal order is key order, and ordinals round-trip
    for kmer in (1, 3, "5p6"):
        ks = (kr.all_kmers(5) + kr.pal6()) if kmer == "5p6" else kr.all_kmers(kmer)
        ords = [kr.ordinal(t, kmer) for t in ks]
        assert len(set(ords)) == len(ks) == kr.n_can(kmer) and max(ords) < kr.ordinal_space(kmer)
        assert [kr.kmer_of_ordinal(o, kmer) for o in ords] == ks
        assert sorted(ks) == [t for _, t in sorted(zip(ords, ks))]


def test_store_cases_take_every_alignment():
    starts = []
    for lead in range(4):
        c = kr.store_case(lead, 0x80)
        starts.append(c.starts)
        at = {}
        for i, p in c.spots.items():
            at.setdefault(len(c.seqs[i]), set()).add(p)
        for L in kr.STORE_LENGTHS[1:]:
            assert {p for p in (0, 15, 16, L - 1, 16 * (L // 16) - 1) if 0 <= p < L} == at[L]
    assert all(set(col.tolist()) == {0, 1, 2, 3} for col in np.array(starts).T[1:])  # all but the lead itself
    lens = {len(s) for s in c.seqs}
    assert set(kr.STORE_LENGTHS) <= lens
    m = kr.many_contigs_case()
    assert m.rounds >= 2 and len(m.seqs) > kr.T.PACK_GRID * kr.T.PRES_WAVES


@pytest.mark.parametrize("kmer", [1, 4, 6, 8, "5p6"])
def test_windows_case(kmer):
    c = kr.windows_case(kmer)
    k = kr.kmin_of(kmer)
    lo, hi = c.each_position
    for p, s in enumerate(c.seqs[lo:hi]):
        assert [i for i, ch in enumerate(s) if ch not in "ACGT"] == [p]
        # windows i <= p < i + k hold the base; i = p - k + 1 has it last, i = p + 1 does not
        hit = [i for i, t in enumerate(kr.kmers_of(s, k)) if not kr.is_acgt(t)]
        assert hit == list(range(max(0, p - k + 1), min(p, 40 - k) + 1))
    assert {(p % 16 + k > 16) for p in range(40)} == {False, True} or k == 1
    lo, hi = c.seams
    spots = {p for s in c.seqs[lo:hi] for p, ch in enumerate(s) if ch not in "ACGT"}
    assert spots == {kr.T.STAGE * m + d for m in (1, 2) for d in (-2, -1, 0, 1)}
    lo, hi = c.tail
    assert {40 - s.index("N") for s in c.seqs[lo:hi]} == set(range(1, max(k, 2)))
    if kmer == "5p6":
        s = c.seqs[c.pal_clean]
        at = [i for i in range(len(s) - 5) if s[i:i + 6] == "ACGGCA"]
        assert any(i // 16 != (i + 5) // 16 for i in at) and any(kr.stage_of(i) != kr.stage_of(i + 5) for i in at)
    agree(c.seqs, kmer)


@pytest.mark.parametrize("with_column", [True, False])
def test_tail_pal_case(with_column):
    c = kr.tail_pal_case(with_column)
    for e in c.ends:
        s = c.seqs[e]
        # what a window reading past the end would see: zero padding (A) or the next contig's first base
        nxt = "A" if len(s) % 16 else c.seqs[e + 1][0]
        assert s[-5:] + nxt == "ACGGCA"
    agree(c.seqs, "5p6")


@pytest.mark.parametrize("kmer,long_contig,odd", [(5, False, False), (5, False, True), ("5p6", False, False),
                                                  ("5p6", False, True), (5, True, False), ("5p6", True, True)])
def test_quotient_case(kmer, long_contig, odd):
    c = kr.quotient_case(kmer, long_contig, odd)
    Q = kr.T.QUOT_TAB
    row = kr.rows(c.seqs, kmer, [c.row])[0]
    assert row[c.pair] == Q - 1 and row[c.pair + 1] == Q and c.pair % 2 == 0
    assert sorted(set(row.values()) & {Q - 2, Q - 1, Q, Q + 1}) == [Q - 2, Q - 1, Q, Q + 1]
    assert c.M % 2 == odd
    assert kr.path_of(c.seqs, kmer) == (kr.WAVE32 if long_contig else kr.WAVE16)
    if not long_contig:
        agree(c.seqs, kmer)


def test_small_row_cases():
    for M in (1, 2, 3):
        c = kr.tiny_m_case(M)
        assert len(kr.columns(c.seqs, 1)) == M
        prof, cols, tot = oracle_profile(c.seqs, 1, kr.key_lens(len(c.seqs)))
        assert cols == kr.columns(c.seqs, 1) and np.array_equal(tot, kr.row_totals(c.seqs, 1))
    for kmer in (4, "5p6"):
        c = kr.row_range_case(kmer)
        assert [i for i, s in enumerate(c.seqs) if not kr.is_acgt(s)] == list(c.exc)
        agree(c.seqs, kmer)
    assert kr.row_aligned(0, 3) and not kr.row_aligned(1, 3) and kr.row_aligned(1, 3, 8) and not kr.row_aligned(0, 4, 8)


def test_choice_cases_sit_on_the_thresholds():
    T = kr.T
    want = {(6, T.WAVE_MAX_M): kr.WAVE16, (6, T.WAVE_MAX_M + 1): kr.BLOCK_LDS, ("5p6", T.WAVE_MAX_M): kr.WAVE16,
            ("5p6", T.WAVE_MAX_M + 1): kr.BLOCK_LDS, (7, 16384): kr.BLOCK_LDS, (7, 16385): kr.BLOCK_LDS,
            (8, T.LDS_COLS): kr.BLOCK_LDS, (8, T.LDS_COLS + 1): kr.BLOCK_SCRATCH}
    assert set(kr.choice_cases()) == set(want)
    for (kmer, M), p in want.items():
        c = kr.choice_case(kmer, M)
        assert c.path == p and len(c.seqs) == M and len(set(c.seqs)) == M
        assert all(len(kr.kmers_of(s, kmer)) == (3 if len(s) == 6 and kmer == "5p6" else 1)
                   for s in c.seqs[:: max(1, M // 500)])
        if M <= T.WAVE_MAX_M + 1 and kmer == 6:
            agree(c.seqs, kmer)
    # k = 8 never takes the wave kernel, whatever M; a long contig makes the wave kernel's counters u32
    assert kr.path(10, kr.ordinal_space(8), 100) == kr.BLOCK_LDS and kr.path(10, 4096, T.U16_LIMIT) == kr.WAVE32
    assert kr.path(10, 4096, T.U16_LIMIT - 1) == kr.WAVE16
    assert 16384 * 4 == 64 * 1024
    for cap, p in ((T.WAVE_MAX_M, kr.WAVE16), (T.WAVE_MAX_M + 1, kr.BLOCK_LDS)):
        c = kr.cap_case(cap)
        assert c.path == p and kr.m_cap(c.seqs, "5p6") == cap
        assert kr.path_of(c.seqs, "5p6") == kr.WAVE16  # on M itself it would be the wave kernel either way
    agree(c.seqs, "5p6")


@pytest.mark.parametrize("kmer,missing6", [(1, False), (3, False), ("5p6", False), ("5p6", True)])
def test_prefix_cases(kmer, missing6):
    P = kr.T.PREFIX
    for where, n in ((P, P + 40), (P + 1, P + 40), (-1, P + 40)):
        c = kr.prefix_case(kmer, where, n=n, missing6=missing6)
        assert c.where == where % n and kr.prefix_ordinals(c.seqs, kmer) == kr.n_can(kmer) - 1
        assert [i for i, s in enumerate(c.seqs) if c.miss in kr.kmers_of(s, kmer)] == [c.where]
        assert (len(c.miss) == 6) == missing6
        full = kr.presence_bits(c.seqs, kmer)
        assert sum(bin(int(w)).count("1") for w in full) == kr.n_can(kmer)
    agree(c.seqs, kmer)


@pytest.mark.parametrize("kmer", [1, 3, "5p6"])
def test_saturated_cases(kmer):
    for inside in (False, True):
        c = kr.saturated_case(kmer, inside)
        assert kr.saturated_after_prefix(c.seqs, kmer) and c.X == len(kr.exception_keys(c.seqs, kmer)) > 0
    agree(c.seqs, kmer)
    c0 = kr.saturated_case(kmer, False, n_exc=0)
    assert c0.X == 0 and all(kr.is_acgt(s) for s in c0.seqs)
    if kmer == "5p6":
        assert kr.saturated_case(kmer, False, n_exc=1).X == 1
        big = kr.saturated_case(kmer, False, n_exc=1500, n=kr.T.PREFIX + 4600)
        assert big.X == 1500 > kr.T.COL_BLOCK


def test_bit_patterns():
    for kmer in (1, 8):
        bits = kr.bit_pattern(kmer)
        S = kr.ordinal_space(kmer)
        ords = kr.ordinals_of_bits(bits)
        assert 0 in ords and S - 1 in ords and S // 4 <= len(ords) < S
        keys = kr.columns_of(bits, np.zeros(0, np.uint64), kmer)
        assert len(keys) == len(ords) and np.all(keys[1:] > keys[:-1])
    assert len(kr.bit_pattern(8)) == 2 * kr.T.COL_BLOCK  # two words per thread of the column table's block
