"""The k-mer side (kmer.hip) stage by stage against tests/kmer_reference.py:
the packed store, the windows with exception bases, the row write, the kernel
choice, the presence passes and the column table.  Every comparison is exact
(u64 views of the doubles); every case asserts from the model that it sits
where it claims, and section D also which kernel runs.

  A  store      ContigStore.words() and the exception-base count against pack()
  B  windows    profile, columns, totals, presence and exception keys
  C  row write  the quotient table's edge, u16 / u32 counters, ld, alignment
  D  choice     M (or the deferred step's capacity) on both sides of each limit
  E  presence   the second pass's saturation test, the column table's merges

Measured on an MI355X: the 65 cases take 3.2 s (the slowest, 40,000 contigs
through the store, 0.3 s).

Single-line mutants of kmer.hip, each built apart and run once against this
module (none is committed).  Every one only changes a value, a comparison or
skips work; "bounds" says why no access leaves its array on this module's
inputs.

  mutant                                   failing cases
  write_row_wave: a >= kQuotTab            C test_quotient_table_edge, all 6
    -> a > kQuotTab                        (count 64 reads the table's entry 63)
    bounds: the index is min(a, 63) either way
  presence_kernel: present >= n_can        E test_last_ordinal_behind_the_prefix,
    -> present + 1 >= n_can                all 12 (the late ordinal's column is gone)
    bounds: scans fewer contigs; each failing case stops at the column
    count, before any profile launch could look up the missing column
  columns_kernel: "if (lo2 >= S) below     B windows[1], E saturated[1-3-*],
    = n_present" dropped                   E chosen_bitmap[1] (S = 4 < 32: a key above
                                           T gets column x + 0)
    bounds: prefix[lo2 >> 5] is prefix[0] or prefix[nwords]; the column
    stays below M
  pack_kernel: mask nibble m4 << (12 - 4q) A all 9 store cases
    -> m4 << 4q                            (run with -k store only)
    bounds: values only; the other sections were not run, a wrong mask
    sends later lookups to columns that do not exist
  write_row_wave: the (M & 1) tail         23 cases of B, C, D, E with odd M
    never taken                            (C quotient[*-True], one_two_and_three[1, 3],
                                           row_ranges, ...)
    bounds: one store and one clear fewer per row
  count_clean: 64 * t + 1 < lim            B test_contig_ending_before_a_palindrome[True]
    -> 64 * t < lim                        (run with -k "ending_before and True")
    bounds: tail_pal_case asserts that the only palindrome a clean contig
    reads on into is ACGGCA, which is a column there; without the column
    (case [False], not run) the add would leave the histogram
  profile_wave_kernel, exception path:     B test_contig_ending_before_a_palindrome[True]
    i + 6 <= L -> true                     (run with -k "ending_before and True")
    bounds: the sixth byte is the next contig's first or the blob's
    padding; the stray 6-mer is ACGGCA, a column (same claim as above)

All seven are caught.  The two end-of-contig mutants were run on case [True]
alone because case [False] has no column for the stray add to land in: there
the row totals would catch it, and the add itself would be out of bounds.
"""
import numpy as np
import pytest

import kmer_reference as kr
from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import ShardedBuild

pytestmark = pytest.mark.gpu

T = kr.T
NAN = np.uint64(0x7FF8DEADBEEF0000)  # a quiet NaN with a payload: what padding must still hold


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


class Plan:
    """A store and a finalized plan over `seqs`, closed on exit."""

    def __init__(self, ctx, seqs, kmer, finalize=True, key_lens=None):
        self.ctx, self.seqs, self.kmer, self.km = ctx, seqs, kmer, kr.kmode_of(kmer)
        self.blob, self.offs, self.key_lens = kr.encode(seqs)
        if key_lens is not None:
            self.key_lens = np.ascontiguousarray(key_lens, np.int32)
        self.store = engine.ContigStore(ctx, self.blob, self.offs, self.key_lens)
        self.plan = engine.KmerPlan(ctx, self.store, self.km)
        self.M = self.plan.finalize() if finalize else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.plan.close()
        self.store.close()

    def presence(self):
        buf = _lib.DevBuf(self.ctx, self.plan.presence_words(), np.uint32)
        self.plan.presence_get(buf.ptr)
        out = buf.numpy()
        buf.close()
        return out

    def exceptions(self):
        n = self.plan.exceptions_count()
        buf = _lib.DevBuf(self.ctx, max(n, 1), np.uint64)
        self.plan.exceptions_get(buf.ptr if n else None)
        out = buf.numpy()[:n]
        buf.close()
        return out

    def rows(self, lo, hi, ld=None):
        out = np.full((hi - lo, ld or self.M), np.nan)
        self.plan.profile_rows(lo, hi, out)
        return out


def model_keys(cols, km):
    return np.array([kr.key_of(t, km) for t in cols], np.uint64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_tables(p, cols=None):
    """Columns, presence bitmap, exception keys and exception bases against the model."""
    cols = kr.columns(p.seqs, p.kmer) if cols is None else cols
    assert p.M == len(cols)
    assert np.array_equal(p.plan.columns(), model_keys(cols, p.km))
    assert np.array_equal(p.presence(), kr.presence_bits(p.seqs, p.kmer))
    assert np.array_equal(p.exceptions(), kr.exception_keys(p.seqs, p.kmer))
    assert p.store.info()["exception_bases"] == sum(ch not in "ACGT" for s in p.seqs for ch in s)
    assert p.plan.profile_path() == kr.path_of(p.seqs, p.kmer, len(cols))
    return cols


def check_rows(p, cols, which):
    """Rows `which`, each read on its own, and their totals."""
    want = kr.rows(p.seqs, p.kmer, which, cols)
    for r, d in zip(which, want):
        got = p.rows(r, r + 1)
        assert same(got[0], kr.dense(d, p.M, int(p.key_lens[r]))), r
        assert p.plan.row_totals()[r] == sum(d.values()), r


def check_all(ctx, seqs, kmer):
    """The whole profile, the tables and the totals."""
    with Plan(ctx, seqs, kmer) as p:
        cols = check_tables(p)
        want = kr.profile(seqs, kmer, p.key_lens, cols)
        assert same(p.plan.profile_host(), want)
        assert np.array_equal(p.plan.row_totals(), kr.row_totals(seqs, kmer))
        return p.plan.profile_path()


# ---- A. the store ---------------------------------------------------------------------
def check_store(store, seqs, blob, offs):
    packed, mask, woff, has_exc, nexc = kr.pack(blob, offs)
    gp, gm, gw, gh = store.words()
    assert np.array_equal(gw, woff)
    bad = np.flatnonzero((gp != packed) | (gm != mask))
    assert not len(bad), (bad[:5], [hex(x) for x in gp[bad[:5]]], [hex(x) for x in packed[bad[:5]]])
    assert np.array_equal(gh != 0, has_exc != 0)
    assert store.info()["exception_bases"] == nexc


@pytest.mark.parametrize("byte", [0x00, 0x80, 0xFF, ord("N")])
def test_store_every_alignment_and_length(ctx, byte):
    for lead in range(4):
        c = kr.store_case(lead, byte)
        blob, offs, kl = kr.encode(c.seqs)
        store = engine.ContigStore(ctx, blob, offs, kl)
        try:
            check_store(store, c.seqs, blob, offs)
        finally:
            store.close()


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_store_from_device_pointers(ctx, shift):
    c = kr.store_case(1, 0x80)
    blob, offs, kl = kr.encode(c.seqs)
    total, n = int(offs[-1]), len(c.seqs)
    slack = 64
    host = np.full(total + 2 * slack + 4, ord("N"), np.uint8)  # exception bytes around the blob: a read of them shows
    host[slack + shift:slack + shift + total] = blob[:total]
    dblob, doffs, dkl = (_lib.DevBuf.from_numpy(ctx, a) for a in (host, offs, kl))
    assert dblob.ptr % 4 == 0 and (dblob.ptr + slack + shift) % 4 == shift
    store = engine.ContigStore(ctx, dblob.ptr + slack + shift, doffs.ptr, dkl.ptr, device_pointers=True, n=n)
    try:
        check_store(store, c.seqs, blob, offs)
    finally:
        store.close()
        for b in (dblob, doffs, dkl):
            b.close()


def test_store_more_contigs_than_one_pack_round(ctx):
    c = kr.many_contigs_case()
    blob, offs, kl = kr.encode(c.seqs)
    store = engine.ContigStore(ctx, blob, offs, kl)
    try:
        check_store(store, c.seqs, blob, offs)
    finally:
        store.close()


# ---- B. windows -----------------------------------------------------------------------
@pytest.mark.parametrize("kmer", [1, 4, 6, 8, "5p6"])
def test_windows_with_exception_bases(ctx, kmer):
    c = kr.windows_case(kmer)
    check_all(ctx, c.seqs, kmer)


@pytest.mark.parametrize("with_column", [True, False])
def test_contig_ending_before_a_palindrome(ctx, with_column):
    c = kr.tail_pal_case(with_column)
    assert check_all(ctx, c.seqs, "5p6") == kr.WAVE16
    # the same ends through the exception path and through the block kernel's window loop
    check_all(ctx, c.exc_seqs, "5p6")
    big = c.seqs + kr.exc_kmers(T.WAVE_MAX_M, 5)
    with Plan(ctx, big, "5p6") as p:
        assert p.plan.profile_path() == kr.BLOCK_LDS
        cols = check_tables(p)
        check_rows(p, cols, c.ends)


# ---- C. the row write -------------------------------------------------------------------
@pytest.mark.parametrize("kmer,long_contig,odd", [(5, False, False), (5, False, True), ("5p6", False, False),
                                                  ("5p6", False, True), (5, True, False), ("5p6", True, True)])
def test_quotient_table_edge(ctx, kmer, long_contig, odd):
    c = kr.quotient_case(kmer, long_contig, odd)
    with Plan(ctx, c.seqs, kmer) as p:
        assert p.plan.profile_path() == (kr.WAVE32 if long_contig else kr.WAVE16)
        cols = check_tables(p)
        assert p.M == c.M and p.M % 2 == odd
        want = kr.profile(c.seqs, kmer, p.key_lens, cols)
        Q, kl = T.QUOT_TAB, int(p.key_lens[c.row])
        assert want[c.row, c.pair] == (Q - 1) / kl and want[c.row, c.pair + 1] == Q / kl
        assert same(p.plan.profile_host(), want)
        assert np.array_equal(p.plan.row_totals(), kr.row_totals(c.seqs, kmer))
        # a device output: ld = M, M + 1, M + 2, the first row on and 8 bytes off a 16-byte boundary
        n, M = len(c.seqs), p.M
        for ld in (M, M + 1, M + 2):
            for base in (0, 8):
                buf = _lib.DevBuf(ctx, n * ld + 2, np.float64)
                assert buf.ptr % 16 == 0
                buf.copy_from(np.full(n * ld + 2, NAN, np.uint64).view(np.float64))
                p.plan.profile_device(buf.ptr + base, ld)
                got = buf.numpy().view(np.uint64)
                buf.close()
                body = got[base // 8:base // 8 + n * ld].reshape(n, ld)
                assert {kr.row_aligned(r, ld, base) for r in range(n)} == ({True, False} if ld % 2 else {base == 0})
                assert np.array_equal(body[:, :M], want.view(np.uint64)), (ld, base)
                assert np.all(body[:, M:] == NAN), (ld, base)
                assert np.all(got[:base // 8] == NAN) and np.all(got[base // 8 + n * ld:] == NAN)


@pytest.mark.parametrize("M", [1, 2, 3])
def test_one_two_and_three_columns(ctx, M):
    c = kr.tiny_m_case(M)
    check_all(ctx, c.seqs, 1)
    with Plan(ctx, c.seqs, 1) as p:
        want = kr.profile(c.seqs, 1, p.key_lens)
        for ld in (M, M + 1):
            got = p.rows(0, len(c.seqs), ld)
            assert same(got[:, :M], want)  # what a host output's padding holds is not specified


@pytest.mark.parametrize("kmer", [4, "5p6"])
def test_row_ranges(ctx, kmer):
    c = kr.row_range_case(kmer)
    n = len(c.seqs)
    with Plan(ctx, c.seqs, kmer) as p:
        cols = check_tables(p)
        want = kr.profile(c.seqs, kmer, p.key_lens, cols)
        tot = kr.row_totals(c.seqs, kmer)
        for lo in (0, 1, 2, 3, 5):
            for hi in (lo + 3, n):
                assert same(p.rows(lo, hi), want[lo:hi]), (lo, hi)
                assert np.array_equal(p.plan.row_totals()[lo:hi], tot[lo:hi])
        for e in c.exc:  # one pass over an exception contig
            assert same(p.rows(e, e + 1), want[e:e + 1])
        empty = np.full((0, p.M), np.nan)
        p.plan.profile_rows(4, 4, empty)  # an empty range


# ---- D. which kernel --------------------------------------------------------------------
@pytest.mark.parametrize("kmer,M", kr.choice_cases())
def test_kernel_choice(ctx, kmer, M):
    c = kr.choice_case(kmer, M)
    n = len(c.seqs)
    with Plan(ctx, c.seqs, kmer) as p:
        assert p.M == M
        assert p.plan.profile_path() == c.path == kr.path(M, kr.ordinal_space(kmer), max(map(len, c.seqs)))
        cols = sorted(c.seqs) if kmer != "5p6" else kr.columns(c.seqs, kmer)
        assert np.array_equal(p.plan.columns(), model_keys(cols, p.km))
        # single rows only: the dense profile is never allocated on either side
        check_rows(p, cols, [r for r in (0, 1, T.PREFIX - 1, T.PREFIX, n - 1) if r < n])
        lo = max(0, n - 40)
        want = kr.rows(c.seqs, kmer, range(lo, n), cols)
        got = p.rows(lo, n)
        for r, d in enumerate(want):
            assert same(got[r], kr.dense(d, M, int(p.key_lens[lo + r])))


@pytest.mark.parametrize("cap", [T.WAVE_MAX_M, T.WAVE_MAX_M + 1])
def test_deferred_step_chooses_on_the_capacity(cap):
    """The deferred step leaves M on the device and sizes the launch by the capacity 1,088 + X."""
    c = kr.cap_case(cap)
    n = len(c.seqs)
    blob, offs, kl = kr.encode(c.seqs)
    cols = kr.columns(c.seqs, "5p6")
    want = kr.profile(c.seqs, "5p6", kl, cols)
    rec = np.ascontiguousarray(engine.synth_records(61, n, 0, 20_000, True))
    ctx = _lib.Context(0)
    build = ShardedBuild(ctx, SoloComm(), -1, n, 0, n)
    store = engine.ContigStore(ctx, blob, offs, kl)
    dev = _lib.DevBuf.from_numpy(ctx, rec.view(np.int64).reshape(-1))
    try:
        plan = engine.KmerPlan(ctx, store, -1)  # the step's own plan has the same store and mode
        assert plan.profile_path(use_cap=True) == c.path == kr.path(cap, kr.ordinal_space("5p6"), 300)
        assert plan.finalize() == len(cols) < cap and plan.profile_path() == kr.WAVE16
        plan.close()
        assert build.native is not None
        for _ in range(2):
            assert build.run(store, dev.ptr, len(rec), count=False)["E_local"] is None
        build.sync()
        assert same(build.native.profile().numpy(), want)
        res = build.run(store, dev.ptr, len(rec), keep=True)
        assert np.array_equal(res["columns"], model_keys(cols, -1))
        assert same(res["profile"].numpy(), want)
    finally:
        build.close()
        store.close()
        dev.close()
        ctx.close()


# ---- E. presence and columns ------------------------------------------------------------
@pytest.mark.parametrize("where", [T.PREFIX, T.PREFIX + 1, -1])
@pytest.mark.parametrize("kmer,missing6", [(1, False), (3, False), ("5p6", False), ("5p6", True)])
def test_last_ordinal_behind_the_prefix(ctx, kmer, missing6, where):
    c = kr.prefix_case(kmer, where, missing6=missing6)
    n = len(c.seqs)
    with Plan(ctx, c.seqs, kmer) as p:
        cols = check_tables(p)
        assert c.miss in cols and p.M == kr.n_can(kmer) + len(kr.exception_keys(c.seqs, kmer))
        check_rows(p, cols, [0, T.PREFIX - 1, T.PREFIX, T.PREFIX + 1, T.PREFIX + 7, c.where, n - 1])


@pytest.mark.parametrize("inside", [False, True])
@pytest.mark.parametrize("kmer,n_exc", [(1, 3), (3, 40), ("5p6", 0), ("5p6", 1), ("5p6", 40), ("5p6", 1500)])
def test_saturated_prefix_and_exception_keys(ctx, kmer, n_exc, inside):
    if n_exc == 1500 and inside:
        c = kr.saturated_case(kmer, True, n_exc=n_exc // 2)  # 3 contigs apart, all inside the prefix
    else:
        c = kr.saturated_case(kmer, inside, n_exc=n_exc, n=T.PREFIX + max(600, 3 * n_exc + 100))
    n = len(c.seqs)
    with Plan(ctx, c.seqs, kmer) as p:
        cols = check_tables(p)
        assert p.plan.exceptions_count() == c.X
        has = [i for i, s in enumerate(c.seqs) if not kr.is_acgt(s)]
        check_rows(p, cols, sorted(set([0, T.PREFIX - 1, T.PREFIX, n - 1] + has[:3] + has[-3:])))


@pytest.mark.parametrize("kmer", [1, 8])
def test_column_table_of_a_chosen_bitmap(ctx, kmer):
    bits = kr.bit_pattern(kmer)
    km = kr.kmode_of(kmer)
    k = kr.kmin_of(kmer)
    for exc in ([], ["\0" * k, "\xff" * k, "A" * (k - 1) + "B", "T" * (k - 1) + "S"]):
        keys = np.array(sorted(kr.key_of(t, km) for t in exc), np.uint64)
        with Plan(ctx, ["A" * k], kmer, finalize=False) as p:
            assert p.plan.presence_words() == len(bits)
            dbits = _lib.DevBuf.from_numpy(ctx, bits)
            dkeys = _lib.DevBuf.from_numpy(ctx, keys[::-1] if len(keys) else np.zeros(1, np.uint64))
            p.plan.presence_set(dbits.ptr)
            p.plan.exceptions_set(dkeys.ptr if len(keys) else None, len(keys))
            p.M = p.plan.finalize()
            want = kr.columns_of(bits, keys, kmer)
            assert p.M == len(want) == len(kr.ordinals_of_bits(bits)) + len(keys)
            assert np.array_equal(p.plan.columns(), want)
            assert np.array_equal(p.presence(), bits) and np.array_equal(p.exceptions(), keys)
            dbits.close()
            dkeys.close()


@pytest.mark.parametrize("kmer", [3, "5p6"])
def test_two_plans_joined_at_the_exchange_points(ctx, kmer):
    c = kr.windows_case(kmer)
    seqs = c.seqs
    h = len(seqs) // 2
    cols = kr.columns(seqs, kmer)
    want = kr.profile(seqs, kmer, kr.key_lens(len(seqs)), cols)
    kl = kr.key_lens(len(seqs))
    with Plan(ctx, seqs[:h], kmer, finalize=False) as a, Plan(ctx, seqs[h:], kmer, finalize=False, key_lens=kl[h:]) as b:
        nw = a.plan.presence_words()
        both = _lib.DevBuf(ctx, 2 * nw, np.uint32)
        a.plan.presence_get(both.ptr)
        b.plan.presence_get(both.ptr + 4 * nw)
        union = np.concatenate([a.exceptions(), b.exceptions()])
        assert len(np.unique(union)) == len(kr.exception_keys(seqs, kmer))
        dkeys = _lib.DevBuf.from_numpy(ctx, union if len(union) else np.zeros(1, np.uint64))
        for p in (a, b):
            p.plan.presence_merge(both.ptr, 2)
            p.plan.exceptions_set(dkeys.ptr if len(union) else None, len(union))
            p.M = p.plan.finalize()
            assert np.array_equal(p.plan.columns(), model_keys(cols, p.km))
        assert same(a.plan.profile_host(), want[:h]) and same(b.plan.profile_host(), want[h:])
        both.close()
        dkeys.close()
