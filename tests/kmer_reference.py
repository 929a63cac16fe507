"""A plain model of the k-mer side (kmer.hip: pack_kernel, presence_kernel,
columns_kernel, profile_wave_kernel, profile_kernel) and inputs that sit on
those kernels' limits.  No device calls and no oracle here:
tests/test_kmer_reference_cpu.py checks the model against the oracle and every
builder against its own claim; tests/test_gpu_kmer_stages.py runs the inputs.

The model is written from the definition, on Python str (latin-1, one code
point per byte): a contig's k-mers are its slices s[i:i + k]; for "5p6" its
5-mers and those 6-mers t with t == t[::-1]; the columns are sorted() of their
union; a row holds count / len(FASTA key), one IEEE division of two exact
doubles.  Rows are sparse ({column: count}), so a row of a profile too large to
allocate can still be asked for.

What it restates of the device code, so that an input lands where it is meant
to: the store's layout in pack(), the u64 column keys in
key_of(), the ACGT ordinals in ordinal(), the kernel choice in path().  The
constants come from the library (karma_kmer_tile) when it is built, so a
retuned kernel moves the cases with it.
"""
import os
import random
import types

import numpy as np

from karma_amd import _lib

DEFAULTS = types.SimpleNamespace(
    STAGE=1024, STAGE_WORDS=65, PAD_WORDS=80, PREFIX=4096, PRES_WAVES=4, PROF_WAVES=8, WAVE_MAX_M=4096,
    WAVE_MAX_S=8192, LDS_COLS=36864, QUOT_TAB=64, U16_LIMIT=65536, COL_BLOCK=1024, PACK_GRID=8192, PRES_GRID=2048)
T = _lib.kmer_tile() if os.path.exists(_lib.LIB_PATH) else DEFAULTS
WAVE16, WAVE32, BLOCK_LDS, BLOCK_SCRATCH = 0, 1, 2, 3
ACGT = "ACGT"
KMERS = (1, 2, 3, 4, 5, 6, 7, 8, "5p6")


# ---- the model ----------------------------------------------------------------------
def kmode_of(kmer):
    return -1 if kmer == "5p6" else int(kmer)


def kmin_of(kmer):
    return 5 if kmer == "5p6" else int(kmer)


def ordinal_space(kmer):
    """S: the ordinals of the presence bitmap."""
    return 5 * 4 ** 5 if kmer == "5p6" else 4 ** int(kmer)


def n_can(kmer):
    """The ACGT ordinals that can occur at all (for 5p6 the 5-mers and the palindromic 6-mers)."""
    return 4 ** 5 + 4 ** 3 if kmer == "5p6" else 4 ** int(kmer)


def kmers_of(s, kmer):
    """Every k-mer occurrence of contig s, in order of position."""
    if kmer != "5p6":
        return [s[i:i + kmer] for i in range(len(s) - kmer + 1)]
    out = [s[i:i + 5] for i in range(len(s) - 4)]
    for i in range(len(s) - 5):
        t = s[i:i + 6]
        if t == t[::-1]:
            out.append(t)
    return out


def columns(seqs, kmer):
    u = set()
    for s in seqs:
        u.update(kmers_of(s, kmer))
    return sorted(u)


def is_acgt(t):
    return all(ch in ACGT for ch in t)


def key_of(t, kmode):
    """The u64 column key: bytes big-endian from bit 63, the length in the low byte unless k = 8."""
    v = 0
    for j, ch in enumerate(t):
        v |= ord(ch) << (56 - 8 * j)
    return v if kmode == 8 else v | len(t)


def kmer_of_key(key, kmode):
    n = 8 if kmode == 8 else key & 0xFF
    return int(key).to_bytes(8, "big")[:n].decode("latin-1")


def ordinal(t, kmer):
    """Bitmap ordinal of an ACGT-only k-mer: its base-4 code; for 5p6 5 * code of the
    first five bases, plus 1 + the sixth base for a 6-mer."""
    code = 0
    for ch in t[:kmin_of(kmer)]:
        code = 4 * code + ACGT.index(ch)
    if kmer != "5p6":
        return code
    return 5 * code + (1 + ACGT.index(t[5]) if len(t) == 6 else 0)


def presence_bits(seqs, kmer):
    bits = np.zeros((ordinal_space(kmer) + 31) // 32, np.uint32)
    for s in seqs:
        for t in set(kmers_of(s, kmer)):
            if is_acgt(t):
                o = ordinal(t, kmer)
                bits[o >> 5] |= np.uint32(1 << (o & 31))
    return bits


def ordinals_of_bits(bits):
    return [32 * w + b for w in range(len(bits)) for b in range(32) if (int(bits[w]) >> b) & 1]


def kmer_of_ordinal(o, kmer):
    k = kmin_of(kmer)
    code, r = (o // 5, o % 5) if kmer == "5p6" else (o, 0)
    t = "".join(ACGT[(code >> (2 * (k - 1 - j))) & 3] for j in range(k))
    return t + ACGT[r - 1] if r else t


def exception_keys(seqs, kmer):
    km = kmode_of(kmer)
    u = set()
    for s in seqs:
        u.update(t for t in kmers_of(s, kmer) if not is_acgt(t))
    return np.array(sorted(key_of(t, km) for t in u), np.uint64)


def columns_of(bits, exc_keys, kmer):
    """The column table of a bitmap and a key list (what finalize builds), as sorted u64 keys."""
    km = kmode_of(kmer)
    keys = [key_of(kmer_of_ordinal(o, kmer), km) for o in ordinals_of_bits(bits)]
    return np.array(sorted(set(keys) | set(int(x) for x in exc_keys)), np.uint64)


def rows(seqs, kmer, which, cols=None):
    """{column index: count} of each contig in `which`."""
    idx = {t: i for i, t in enumerate(columns(seqs, kmer) if cols is None else cols)}
    out = []
    for r in which:
        d = {}
        for t in kmers_of(seqs[r], kmer):
            d[idx[t]] = d.get(idx[t], 0) + 1
        out.append(d)
    return out


def dense(row, M, key_len):
    v = np.zeros(M, np.float64)
    for c, n in row.items():
        v[c] = n / key_len
    return v


def profile(seqs, kmer, key_lens, cols=None):
    cols = columns(seqs, kmer) if cols is None else cols
    rr = rows(seqs, kmer, range(len(seqs)), cols)
    out = np.zeros((len(seqs), len(cols)), np.float64)
    for r, d in enumerate(rr):
        out[r] = dense(d, len(cols), int(key_lens[r]))
    return out


def row_totals(seqs, kmer):
    return np.array([len(kmers_of(s, kmer)) for s in seqs], np.int64)


def encode(seqs):
    """(blob uint8 with 16 zero bytes behind it, offsets, default key lengths) of the engine's layout."""
    vals = [s.encode("latin-1") for s in seqs]
    offs = np.zeros(len(vals) + 1, np.int64)
    if vals:
        np.cumsum([len(v) for v in vals], out=offs[1:])
    blob = np.frombuffer(b"".join(vals) + b"\0" * 16, np.uint8)
    return blob, offs, key_lens(len(seqs))


def key_lens(n):
    """Key lengths 1 ... 7 in turn, so rows divide by different numbers."""
    return (1 + np.arange(n) % 7).astype(np.int32)


def pack(blob, offs):
    """The store: (packed uint32[W], mask uint16[W], word offsets int64[n + 1], exception
    flag uint8[n], exception bases).  16 bases per word, first base in bits 31:30, A C G T
    = 0 1 2 3, anything else 0 with bit 15 - j of the mask word set; every contig starts
    on a word; bases past a contig's end are 0 and unmasked."""
    blob, offs = np.asarray(blob, np.uint8), np.asarray(offs, np.int64)
    n = len(offs) - 1
    woff = np.zeros(n + 1, np.int64)
    np.cumsum((np.diff(offs) + 15) // 16, out=woff[1:])
    code = np.zeros(256, np.uint32)
    exc = np.ones(256, np.uint32)
    for v, ch in enumerate(ACGT):
        code[ord(ch)], exc[ord(ch)] = v, 0
    packed, mask = np.zeros(woff[-1], np.uint32), np.zeros(woff[-1], np.uint16)
    has_exc = np.zeros(n, np.uint8)
    sh2 = (30 - 2 * np.arange(16)).astype(np.uint32)
    sh1 = (15 - np.arange(16)).astype(np.uint32)
    for c in range(n):
        b = blob[offs[c]:offs[c + 1]]
        if not len(b):
            continue
        nw = woff[c + 1] - woff[c]
        cw, ew = np.zeros(16 * nw, np.uint32), np.zeros(16 * nw, np.uint32)
        cw[:len(b)], ew[:len(b)] = code[b], exc[b]
        packed[woff[c]:woff[c + 1]] = (cw.reshape(nw, 16) << sh2).sum(axis=1, dtype=np.uint32)
        mask[woff[c]:woff[c + 1]] = (ew.reshape(nw, 16) << sh1).sum(axis=1, dtype=np.uint32).astype(np.uint16)
        has_exc[c] = ew.any()
    return packed, mask, woff, has_exc, int(exc[blob[offs[0]:offs[-1]]].sum())


# ---- where an input sits --------------------------------------------------------------
def path(M, S, max_len):
    """The kernel karma_kmer_profile launches (karma_kmer_profile_path)."""
    if M <= T.WAVE_MAX_M and S <= T.WAVE_MAX_S:
        return WAVE16 if max_len < T.U16_LIMIT else WAVE32
    return BLOCK_LDS if M <= T.LDS_COLS else BLOCK_SCRATCH


def path_of(seqs, kmer, M=None):
    M = len(columns(seqs, kmer)) if M is None else M
    return path(M, ordinal_space(kmer), max((len(s) for s in seqs), default=0))


def m_cap(seqs, kmer):
    """The deferred step's column capacity: every ACGT ordinal that can occur plus the exception keys."""
    return n_can(kmer) + len(exception_keys(seqs, kmer))


def stage_of(pos):
    return pos // T.STAGE


def row_aligned(r, ld, base=0):
    """Row r of an output whose first byte is `base` bytes off a 16-byte boundary starts on one."""
    return (base + 8 * r * ld) % 16 == 0


def prefix_ordinals(seqs, kmer):
    return int(sum(bin(int(w)).count("1") for w in presence_bits(seqs[:T.PREFIX], kmer)))


def saturated_after_prefix(seqs, kmer):
    return prefix_ordinals(seqs, kmer) >= n_can(kmer)


def rand_acgt(rng, n):
    return "".join(rng.choice(ACGT) for _ in range(n))


def all_kmers(k):
    return [kmer_of_ordinal(o, k) for o in range(4 ** k)]


def pal6():
    """The 64 palindromic ACGT 6-mers."""
    return [t + t[::-1] for t in all_kmers(3)]


def case(seqs, kmer, **claims):
    return types.SimpleNamespace(seqs=list(seqs), kmer=kmer, **claims)


# ---- A. the store --------------------------------------------------------------------
STORE_LENGTHS = tuple(range(41)) + (63, 64, 65, 1023, 1024, 1025)


def store_case(lead, byte, lengths=STORE_LENGTHS, seed=3):
    """Contigs of every length in `lengths`, clean and with the exception byte `byte` at
    base 0, 15, 16, the last base and the last base of the last full word; a leading
    contig of `lead` bytes shifts every start, so the four leads give every contig every
    alignment; empty contigs first (lead 0), in the middle and last."""
    rng = random.Random(seed)
    ch = chr(byte)
    seqs = [rand_acgt(rng, lead)]
    spots = {}
    for L in lengths:
        s = rand_acgt(rng, L)
        seqs.append(s)
        for p in sorted({0, 15, 16, L - 1, 16 * (L // 16) - 1}):
            if 0 <= p < L:
                spots[len(seqs)] = p
                seqs.append(s[:p] + ch + s[p + 1:])
        if L == 20:
            seqs.append("")
    seqs.append("")
    blob, offs, _ = encode(seqs)
    assert offs[1] == lead and (lead or seqs[0] == "") and seqs[-1] == "" and "" in seqs[1:-1]
    for c, p in spots.items():
        assert seqs[c][p] == ch and sum(x not in ACGT for x in seqs[c]) == 1
    # both branches of pack_kernel's loads: a word whose 20-byte window lies inside the contig, and a last word
    assert any(len(s) >= 16 + 20 for s in seqs) and any(0 < len(s) % 16 < 4 for s in seqs)
    return case(seqs, None, starts=offs[:-1] % 4, spots=spots)


def many_contigs_case(n=40000, seed=5):
    """More contigs than one round of pack_kernel's largest grid has waves, 8 bases each, an
    exception base in every 97th."""
    rng = random.Random(seed)
    seqs = [rand_acgt(rng, 8) for _ in range(n)]
    for c in range(0, n, 97):
        seqs[c] = seqs[c][:c % 8] + "N" + seqs[c][c % 8 + 1:]
    assert n > T.PACK_GRID * T.PRES_WAVES  # pack_kernel's blocks have as many waves as the presence pass's
    return case(seqs, 8, rounds=-(-n // (T.PACK_GRID * T.PRES_WAVES)))


# ---- B. windows ----------------------------------------------------------------------
EXC_BYTES = "NnRY\r-*\x00\x80\xff"


def windows_case(kmer, seed=7):
    """Exception bases against every window edge: one at each position of a 40-base
    contig (inside and outside each window, o + k on both sides of 16); at 1,022 ...
    1,025 and 2,046 ... 2,049 of a 3,100-base contig (the stage seams); in the last
    k - 1 bases; for 5p6 a clean 5-mer before an exception 6th base, exception
    palindromes, and a clean palindrome across a word edge and a stage edge."""
    rng = random.Random(seed)
    k = kmin_of(kmer)
    seqs, claims = [], {}
    base40 = rand_acgt(rng, 40)
    seqs.append(base40)
    for p in range(40):
        seqs.append(base40[:p] + EXC_BYTES[p % len(EXC_BYTES)] + base40[p + 1:])
    claims["each_position"] = (1, 41)
    long = rand_acgt(rng, 3100)
    seams = [T.STAGE - 2, T.STAGE - 1, T.STAGE, T.STAGE + 1, 2 * T.STAGE - 2, 2 * T.STAGE - 1, 2 * T.STAGE,
             2 * T.STAGE + 1]
    claims["seams"] = (len(seqs), len(seqs) + len(seams) + 1)
    for p in seams:
        seqs.append(long[:p] + "N" + long[p + 1:])
    s = list(long)
    for p in seams[::2]:
        s[p] = "\x00"
    seqs.append("".join(s))
    assert {stage_of(p) for p in seams} == {0, 1, 2} and len(long) > 3 * T.STAGE
    claims["tail"] = (len(seqs), len(seqs) + max(k - 1, 1))
    for j in range(1, max(k, 2)):  # the exception base j bases before the end
        seqs.append(base40[:40 - j] + "N" + base40[41 - j:])
        assert seqs[-1][40 - j] == "N" and len(seqs[-1]) == 40
    if kmer == "5p6":
        extra = ["ACGTAN", "GG" + "ACGTA" + "N" + "CC", "N\0\0\0\0N", "\0ACCA\0", "nACCAn",
                 "AC" + "N\0\0\0\0N" + "GT", "T\0ACCA\0T", "GnACCAnG", "\0\0\0\0\0\0\0", "\0" * 5]
        claims["pal_exc"] = (len(seqs), len(seqs) + len(extra))
        seqs += extra
        got = columns(extra, kmer)
        for t in ("N\0\0\0\0N", "\0ACCA\0", "nACCAn", "\0" * 6, "\0" * 5):
            assert t in got
        assert "ACGTAN" not in got and "ACGTA" in got
        # a clean palindrome whose window crosses a word edge (13 ... 18) and a stage edge (1,021 ... 1,026)
        body = list(rand_acgt(rng, 1100))
        for p in (13, T.STAGE - 3):
            body[p:p + 6] = "ACGGCA"
            assert p // 16 != (p + 5) // 16
        assert stage_of(T.STAGE - 3) != stage_of(T.STAGE + 2)
        claims["pal_clean"] = len(seqs)
        seqs.append("".join(body))
        seqs.append("".join(body[:500]) + "N" + "".join(body[501:]))  # the same through the exception path
        assert kmers_of(seqs[-1], kmer).count("ACGGCA") >= 2
    return case(seqs, kmer, **claims)


def overrun_6mers(seqs):
    """What a 6-mer window at each clean contig's last 5-mer would read: the contig's last
    five bases and the zero padding of its last word (A), or the next contig's first base."""
    out = []
    for c, s in enumerate(seqs):
        if len(s) >= 5 and is_acgt(s):
            nxt = "A" if len(s) % 16 or c + 1 == len(seqs) or not seqs[c + 1] else seqs[c + 1][0]
            out.append(s[-5:] + nxt)
    return out


def tail_pal_case(with_column, seed=11):
    """5p6: contigs that end in ACGGC, whose last 5-mer would read on as the palindrome
    ACGGCA into the zero padding of a partly filled word (L % 16 = 5, 15) or into the
    next contig's first base (L % 16 = 0, the next one begins with A).  with_column: the
    column ACGGCA exists through another contig, so a stray add would land in the row;
    without it the row totals catch it."""
    rng = random.Random(seed)
    seqs, ends = [], []
    for L in (32, 21, 31, 1024, 16, 5):
        while True:
            s = rand_acgt(rng, L - 5) + "ACGGC"
            if "ACGGCA" not in s:
                break
        ends.append(len(seqs))
        seqs.append(s)
        while True:
            f = "A" + rand_acgt(rng, 9) if L % 16 == 0 else rand_acgt(rng, 7)
            if "ACGGCA" not in f:
                break
        seqs.append(f)
    if with_column:
        seqs.append("TTACGGCATT")
    for c in ends:
        assert seqs[c].endswith("ACGGC") and "ACGGCA" not in kmers_of(seqs[c], "5p6")
        if len(seqs[c]) % 16 == 0:
            assert seqs[c + 1][0] == "A"
    assert {len(seqs[c]) % 16 for c in ends} == {0, 5, 15}
    assert ("ACGGCA" in columns(seqs, "5p6")) == with_column
    # the same ends behind an exception base: the windows go through the byte-key path
    exc = [s if i not in ends else "N" + s[1:] for i, s in enumerate(seqs)]
    for ss in (seqs, exc):
        cols = columns(ss, "5p6")
        over = [t for t in overrun_6mers(ss) if t == t[::-1]]
        # no clean contig but the chosen ones reads on into a palindrome; with the column present, a stray
        # add of theirs has a column to land in
        assert set(over) <= {"ACGGCA"} and (not with_column or "ACGGCA" in cols)
    return case(seqs, "5p6", ends=ends, exc_seqs=exc)


# ---- C. the row write ------------------------------------------------------------------
def quotient_case(kmer, long_contig=False, odd=False, seed=13):
    """Counts QUOT_TAB - 2 ... QUOT_TAB + 1 in row `row`: below the table's end, its last
    entry, and the first two counts that are divided; QUOT_TAB - 1 | QUOT_TAB in the low
    and high half of one u16 pair (columns 2j, 2j + 1).  long_contig: a contig of
    U16_LIMIT bases in the store, which makes every counter u32.  odd: M is odd."""
    assert kmer in (5, "5p6")
    Q = T.QUOT_TAB
    rng = random.Random(seed)
    # runs joined by bytes whose k-mers sort outside (AAAAA, CCCCC): '*' < 'A', 'n' > 'T'
    if kmer == 5:
        a, c, g, t = Q - 1 + 4, Q + 4, Q - 2 + 4, Q + 1 + 4  # AAAAA Q-1, CCCCC Q, GGGGG Q-2, TTTTT Q+1
        lo, hi = "AAAAA", "CCCCC"
    else:
        a, c, g, t = Q - 1 + 5, Q + 4, Q - 2 + 5, Q + 1 + 5  # AAAAAA Q-1, CCCCC Q, GGGGGG Q-2, TTTTTT Q+1
        lo, hi = "AAAAAA", "CCCCC"
    main = "A" * a + "*" + "C" * c + "n" + "G" * g + "n" + "T" * t
    # the other contigs hold G and T only: no column of theirs falls between the pair's
    gt = lambda n: "".join(rng.choice("GT") for _ in range(n))
    others = ["*AAAA", "GGTTGTGTTNGG", gt(50), "", "TTGTTGT"]
    if long_contig:
        others.append(gt(T.U16_LIMIT))
    for shift in ([], ["*ACGT"], ["nnnnn"], ["*ACGT", "nnnnn"]):  # a column before the pair, one behind it
        seqs = [others[0], main] + others[1:] + shift
        cols = columns(seqs, kmer)
        if cols.index(lo) % 2 == 0 and (len(cols) % 2 == 1) == odd:
            break
    else:
        raise AssertionError("no column shift puts the pair on an even column")
    row = rows(seqs, kmer, [1], cols)[0]
    j = cols.index(lo)
    assert cols[j + 1] == hi and j % 2 == 0 and row[j] == Q - 1 and row[j + 1] == Q
    assert {Q - 2, Q - 1, Q, Q + 1} <= set(row.values())
    assert (max(len(s) for s in seqs) >= T.U16_LIMIT) == long_contig and (len(cols) % 2 == 1) == odd
    return case(seqs, kmer, row=1, pair=j, M=len(cols))


def tiny_m_case(M):
    """k = 1 with M = 1, 2 or 3 columns."""
    seqs = {1: ["AAAA", "A", "AA"], 2: ["ACAC", "C", "", "AAC"], 3: ["ACG", "GGA", "C", "", "GCA"]}[M]
    assert len(columns(seqs, 1)) == M
    return case(seqs, 1, M=M)


def row_range_case(kmer, seed=17):
    """Twelve contigs, exception bases in 1, 2, 6 and 7: row ranges that start at 0, 1, 2, 3
    and 5 read the flag bytes from every position of a dword."""
    rng = random.Random(seed)
    seqs = [rand_acgt(rng, 30 + 7 * i) for i in range(12)]
    for c in (1, 2, 6, 7):
        seqs[c] = seqs[c][:9 + c] + "N" + seqs[c][10 + c:]
    return case(seqs, kmer, exc=(1, 2, 6, 7))


# ---- D. which kernel -------------------------------------------------------------------
EXC2 = "\x00\r*-NRYn\x80\xff"


def exc_kmers(n, k):
    """n distinct k-mers (k >= 3) of two exception bytes and ACGT."""
    out = []
    for x in EXC2:
        for y in EXC2:
            for t in all_kmers(min(k - 2, 3)):
                out.append(x + y + t + "A" * (k - 2 - len(t)))
    assert n <= len(out) == len(set(out))
    return out[:n]


def choice_case(kmer, M):
    """Exactly M columns, one contig per k-mer (5p6: per 5-mer and per palindromic 6-mer),
    then one contig per exception k-mer for what M has beyond the ACGT ordinals."""
    k = kmin_of(kmer)
    seqs = (all_kmers(5) + pal6()) if kmer == "5p6" else all_kmers(k)
    if M <= len(seqs):
        seqs = seqs[:M]
    else:
        seqs = seqs + exc_kmers(M - len(seqs), k)
    got = M if len(seqs) > 20000 else len(columns(seqs, kmer))  # distinct k-mers, one per contig
    assert got == M == len(set(seqs))
    return case(seqs, kmer, M=M, path=path(M, ordinal_space(kmer), k + 1))


def choice_cases():
    """(k, M) on both sides of every threshold of the kernel choice."""
    out = [(6, T.WAVE_MAX_M), (6, T.WAVE_MAX_M + 1), ("5p6", T.WAVE_MAX_M), ("5p6", T.WAVE_MAX_M + 1),
           (7, 16384), (7, 16385), (8, T.LDS_COLS), (8, T.LDS_COLS + 1)]
    return out


def cap_case(cap):
    """5p6 whose column capacity 1,088 + X is `cap` while M stays far below it."""
    X = cap - n_can("5p6")
    seqs = [rand_acgt(random.Random(19), 300)] + exc_kmers(X, 5)
    assert m_cap(seqs, "5p6") == cap and len(columns(seqs, "5p6")) < cap - 500
    return case(seqs, "5p6", cap=cap, path=path(cap, ordinal_space("5p6"), 300))


# ---- E. presence and columns -----------------------------------------------------------
def prefix_case(kmer, where, n=9000, missing6=False, seed=23):
    """The first PREFIX contigs hold every ACGT ordinal but one; that one occurs only in
    contig `where` (an index >= PREFIX, or -1: the last), which has ACGT only.  Contigs
    behind the prefix repeat the prefix's; every 50th has an exception base."""
    k = kmin_of(kmer)
    if kmer == "5p6":
        units = all_kmers(5) + pal6()
        miss = "GACCAG" if missing6 else "ACGTA"  # no palindromic 6-mer contains ACGTA
    else:
        units = all_kmers(k)
        miss = units[-2] if len(units) > 1 else units[0]
    units = [u for u in units if u != miss]
    where = where % n
    seqs = [units[i % len(units)] for i in range(n)]
    for c in range(T.PREFIX + 7, n, 50):
        if c != where:
            seqs[c] = "N" + seqs[c][1:]
    seqs[where] = miss
    assert where >= T.PREFIX and is_acgt(seqs[where])
    assert prefix_ordinals(seqs, kmer) == n_can(kmer) - 1 and not saturated_after_prefix(seqs, kmer)
    assert sum(miss in kmers_of(s, kmer) for s in seqs) == 1
    assert prefix_ordinals([seqs[where]] + seqs, kmer) == n_can(kmer)
    return case(seqs, kmer, where=where, miss=miss)


def saturated_case(kmer, exc_inside, n_exc=40, n=None, seed=29):
    """A prefix that holds every ACGT ordinal; the contigs with exception bases all lie
    behind it (exc_inside False) or all inside it (True).  The exception keys sort below
    the first ordinal's (NUL), between two adjacent ordinals' and above the last one's
    (0xFF)."""
    k = kmin_of(kmer)
    units = (all_kmers(5) + pal6()) if kmer == "5p6" else all_kmers(k)
    n = n or T.PREFIX + 600
    seqs = [units[i % len(units)] for i in range(n)]
    mid = units[len(units) // 2]
    special = ["\0" * k, "\xff" * k, mid[:-1] + "B" if mid[-1] == "A" else mid[:-1] + chr(ord(mid[-1]) + 1)]
    excs = list(dict.fromkeys(special + [t[:k] for t in exc_kmers(max(n_exc - 3, 0), max(k, 3))]))[:n_exc]
    at = range(5, 5 + 3 * len(excs), 3) if exc_inside else range(n - 3 * len(excs), n, 3)
    for c, t in zip(at, excs):
        seqs[c] = t
    has = [c for c, s in enumerate(seqs) if not is_acgt(s)]
    assert saturated_after_prefix(seqs, kmer)
    assert all(c < T.PREFIX for c in has) if exc_inside else all(c >= T.PREFIX for c in has)
    keys = exception_keys(seqs, kmer)
    km = kmode_of(kmer)
    if n_exc >= 3:
        ords = [key_of(t, km) for t in sorted(units)]
        x = key_of(special[2], km)
        assert keys[0] < ords[0] and keys[-1] > ords[-1]
        assert any(a < x < b for a, b in zip(ords, ords[1:])) and x in keys.tolist()
    return case(seqs, kmer, X=len(keys))


def bit_pattern(kmer):
    """Half of the ordinals (at least): the first and last bit of a word, the first and
    last word, an empty word."""
    S = ordinal_space(kmer)
    nw = (S + 31) // 32
    bits = np.zeros(nw, np.uint32)
    if nw == 1:  # k = 1, 2: four or sixteen ordinals
        bits[0] = 0b1001 if S == 4 else 0x8001 | 0x0FF0
        return bits
    rng = np.random.default_rng(31)
    bits[:] = rng.integers(0, 1 << 32, nw, dtype=np.uint64).astype(np.uint32)
    bits[0] |= 1
    bits[nw - 1] |= np.uint32(1 << 31)
    bits[1] = 0x80000001
    bits[nw // 2] = 0
    bits[nw // 2 + 1] = 0xFFFFFFFF
    assert bits[0] & 1 and bits[-1] >> 31 and not bits[nw // 2]
    return bits
