"""GPU parity: the HIP path (through libkarma_hip.so) vs the reference.

Two references are used:
  * tests/golden/golden.json — outputs of lmfaber/karma itself (captured by
    tests/golden/make_golden.py), compared through the drop-in classes;
  * oracle/ — the CPU restatement pinned by those goldens, for seeded inputs
    larger than the goldens (bit-exact integer counts and f64 weights).
Everything here is bit-exact: integer counts, and f64 values that are one IEEE
division (profile) or two divisions, one add and one halving (weights).
"""
import ctypes
import hashlib
from collections import OrderedDict

import numpy as np
import pytest

from karma_amd import _lib, engine, synth
from karma_amd.contig import Contig
from karma_amd.kmer import KmerClustering
from karma_amd.read_graph import ReadGraph
from oracle import oracle
from record_layouts import chunk_edge_records

pytestmark = pytest.mark.gpu


def calc(seqs, kmer):
    k = KmerClustering(OrderedDict(seqs), "/tmp", kmer, 4)
    return k, k._KmerClustering__calc_kmer_profile()


def check_profile(out, seqs, kmer):
    if "exit" in out:
        with pytest.raises(SystemExit) as e:
            calc(seqs, kmer)
        assert e.value.code == out["exit"]
        return
    if "raises" in out:
        with pytest.raises(Exception) as e:
            calc(seqs, kmer)
        assert type(e.value).__name__ == out["raises"]
        return
    k, prof = calc(seqs, kmer)
    assert prof.dtype == np.float64
    assert list(prof.shape) == out["shape"]
    assert [km for km, _ in sorted(k.kmers.items(), key=lambda kv: kv[1])] == out["columns"]
    assert k.sorted_kmer_set == []
    assert hashlib.sha256(prof.astype("<f8").tobytes()).hexdigest() == out["sha256"]
    if "nz" in out:
        r, c = prof.nonzero()
        assert [[int(a), int(b), float(prof[a, b])] for a, b in zip(r, c)] == out["nz"]


def test_profile_golden_hand(golden):
    for name, case in golden["profile_hand"].items():
        check_profile(case["out"], [tuple(x) for x in case["seqs"]], case["kmer"])


def test_profile_golden_random(golden):
    for name, case in golden["profile_rand"].items():
        seqs = synth.contig_sequences(case["seed"], case["n"], case["len_min"], case["len_span"], case["n_rate"])
        check_profile(case["out"], list(seqs.items()), case["kmer"])


def test_profile_golden_config1(golden):
    case = golden["profile_config1"]
    seqs = synth.contig_sequences(case["seed"], case["n"])
    check_profile(case["out"], list(seqs.items()), case["kmer"])


@pytest.mark.parametrize("kmer,n_rate", [("5p6", 0), ("5p6", 50), (5, 30), (7, 0), (7, 100), (3, 5), (1, 9),
                                         (8, 0), (8, 200), (4, 0), (6, 64)])
def test_profile_vs_oracle_seeded(kmer, n_rate):
    seed = 100 + sum(map(ord, str(kmer))) % 7 + n_rate
    blob, offs, key_len = engine.synth_contigs(seed, 1500, 20, 1500, n_rate)
    seqs = OrderedDict((f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(1500))
    prof, cols, tot = engine.kmer_profile(seqs, kmer)
    oprof, ocols, ocounts = oracle.calc_kmer_profile(seqs, kmer)
    assert cols == ocols
    assert prof.shape == oprof.shape
    assert np.array_equal(prof.view(np.uint64), oprof.view(np.uint64))
    assert np.array_equal(tot, ocounts.sum(axis=1))


def test_profile_lowercase_iupac_and_bytes():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgtRY\r-*", np.uint8)
    seqs = OrderedDict()
    for i in range(300):
        L = int(rng.integers(6, 400))
        seqs[f">s{i} desc"[: 2 + i % 9]] = bytes(alphabet[rng.integers(0, len(alphabet), L)]).decode("latin-1")
    for kmer in ("5p6", 5, 2, 7, 8):
        prof, cols, _ = engine.kmer_profile(seqs, kmer)
        oprof, ocols, _ = oracle.calc_kmer_profile(seqs, kmer)
        assert cols == ocols
        assert np.array_equal(prof.view(np.uint64), oprof.view(np.uint64))


def test_profile_long_contigs_and_large_k8_columns():
    # k=8 with every 8-mer present -> M > LDS capacity: global-scratch variant
    blob, offs, key_len = engine.synth_contigs(77, 40, 30000, 20000, 0)
    seqs = OrderedDict((f">c{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(40))
    prof, cols, _ = engine.kmer_profile(seqs, 8)
    oprof, ocols, _ = oracle.calc_kmer_profile(seqs, 8)
    assert len(cols) > 36 * 1024
    assert cols == ocols
    assert np.array_equal(prof.view(np.uint64), oprof.view(np.uint64))


@pytest.mark.parametrize("L", [65_535, 65_536])  # the last u16 case, the first u32 case
@pytest.mark.parametrize("kmer", [1, 2, 5, "5p6"])
def test_profile_u16_counters_at_their_limit(kmer, L):
    """profile_wave_kernel packs two u16 counters per u32 while every contig is
    shorter than 2^16 bases (kmer.hip C16), right only because a count is at
    most L.  Long contigs at that limit put maximal counts into one counter
    (poly-A: at k = 1 and L = 65,535 the count is 0xFFFF exactly) and
    near-maximal ones into counters of neighbouring columns, the two halves of
    one u32 (AC repeated; half poly-A, half poly-C), among 200 short contigs.
    Each long contig stands first, in the middle and last once (a wave
    strides over contigs).  Bit-exact against the oracle: profile, columns,
    row totals."""
    blob, offs, _ = engine.synth_contigs(88, 200, 30, 870, 300)
    short = [(f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(200)]
    long_ = [(">polyA", "A" * L), (">AC", ("AC" * (L // 2 + 1))[:L]), (">halves", "A" * (L // 2) + "C" * (L - L // 2))]
    assert all(len(s) == L for _, s in long_)
    for rot in range(3):
        first, mid, last = (long_[(rot + i) % 3] for i in range(3))
        seqs = OrderedDict([first] + short[:100] + [mid] + short[100:] + [last])
        assert len(seqs) == 203
        prof, cols, tot = engine.kmer_profile(seqs, kmer)
        oprof, ocols, ocounts = oracle.calc_kmer_profile(seqs, kmer)
        assert cols == ocols
        assert prof.shape == oprof.shape
        assert np.array_equal(prof.view(np.uint64), oprof.view(np.uint64)), (rot, kmer, L)
        assert np.array_equal(tot, ocounts.sum(axis=1))
        if kmer == 1:  # the count the test is about did occur: L x 'A' in the poly-A row
            assert int(ocounts[list(seqs).index(">polyA")].max()) == L


def test_profile_unsupported_k_raises():
    with pytest.raises(_lib.KarmaError):
        engine.kmer_profile(OrderedDict([(">a", "ACGTACGTACGT")]), 9)


# ---------------------------------------------------------------- graphs ----

def dump(g):
    return {"nodes": [str(n) for n in g.nodes()],
            "edges": [[str(a), str(b), float(d["weight"])] for a, b, d in g.edges(data=True)]}


def test_eq_graph_golden(golden, tmp_path):
    for name, case in list(golden["eq_hand"].items()):
        p = tmp_path / f"{name}.txt"
        p.write_text(case["text"])
        out = case["out"]
        if "raises" in out:
            with pytest.raises(Exception) as e:
                ReadGraph.from_equivalence_classes(str(p), OrderedDict((k, "") for k in case["fasta"]))
            assert type(e.value).__name__ == out["raises"], name
            continue
        g = ReadGraph.from_equivalence_classes(str(p), OrderedDict((k, "") for k in case["fasta"]))
        assert isinstance(g, ReadGraph)
        d = dump(g)
        assert d["edges"] == out["edges"], name
        n_txp = int(case["text"].split("\n")[0])
        assert d["nodes"][:n_txp] == out["nodes"][:n_txp]
        assert set(d["nodes"]) == set(out["nodes"])
    for name, case in golden["eq_synth"].items():
        classes = synth.eq_classes(case["seed"], case["n"], case["n_frags"], case["paired"])
        names = [f"ctg{i}" for i in range(case["n"])]
        p = tmp_path / f"{name}.txt"
        p.write_text(synth.eq_file_text(names, classes))
        d = dump(ReadGraph.from_equivalence_classes(str(p), OrderedDict((">" + x, "") for x in names)))
        assert d["edges"] == case["out"]["edges"]
        assert d["nodes"] == case["out"]["nodes"]


def make_contigs(names, readsets):
    out = []
    for n, reads in zip(names, readsets):
        c = Contig(n)
        c.load_from_iterator([f"{r}\t0\t{n}\t1\t60\t*" for r in reads])
        out.append(c)
    return out


def test_readset_graph_golden(golden):
    for name, case in golden["readset_hand"].items():
        g = ReadGraph.from_contigs(make_contigs(case["names"], case["readsets"]))
        assert dump(g) == case["out"], name
    for name, case in golden["readset_synth"].items():
        recs = synth.read_records(case["seed"], case["n"], case["n_frags"], case["paired"])
        sets = [[] for _ in range(case["n"])]
        for r, c in recs:
            sets[c].append(f"r{r}")
        g = ReadGraph.from_contigs(make_contigs([f"ctg{i}" for i in range(case["n"])], sets))
        assert dump(g) == case["out"], name


def test_update_graph_golden(golden):
    for name, case in golden["update_hand"].items():
        g = ReadGraph()
        for a, b, w in case["base_edges"]:
            g.add_edge(a, b, weight=w)
        g.set_original_contigs(make_contigs(case["orig_names"], case["orig_sets"]))
        g.update_graph(make_contigs(case["new_names"], case["new_sets"]))
        assert dump(g) == case["out"], name


def check_records(rec, n, grouped=True, flagged=True):
    """The HIP graph of (read, contig) records against the oracle; grouped
    records also as KARMA_REC_FLAGGED words (engine.flag_records: read ids
    replaced by read-start flags, 4 bytes per record), which must give the
    same graph bit for bit."""
    e = engine.graph_from_records(rec, n, grouped=grouped)
    rs = np.asarray(rec, dtype=np.int64)
    order = np.argsort(rs[:, 0], kind="stable")
    rs = rs[order]
    starts = np.flatnonzero(np.r_[True, rs[1:, 0] != rs[:-1, 0]]) if len(rs) else np.zeros(0, np.int64)
    off = np.r_[starts, len(rs)]
    o = oracle.graph_groups(off, rs[:, 1] if len(rs) else np.zeros(0), None, None, n, dedup=True)
    outs = [e]
    if grouped and flagged:
        outs.append(engine.graph_from_records(engine.flag_records(rec), n, flagged=True))
    for x in outs:
        assert np.array_equal(x.a, o["a"])
        assert np.array_equal(x.b, o["b"])
        assert np.array_equal(x.shared, o["shared"])
        assert np.array_equal(x.weight.view(np.uint64), o["weight"].view(np.uint64))
        assert np.array_equal(x.totals, o["totals"])
    return e


@pytest.mark.parametrize("seed,n,nf,paired", [(2, 20_000, 400_000, True), (5, 3_000, 200_000, False),
                                              (9, 777, 50_000, True), (4, 1, 1000, True),
                                              # wide partition variants (> 512 pair / > 128 code buckets),
                                              # config 5's 1M contigs, 8 x 200k (weak-scaled config 3), and
                                              # past 2^21 (no compact path)
                                              (10, 600_000, 1_000_000, True), (11, 1_000_000, 2_000_000, True),
                                              (12, 1_100_000, 1_000_000, True), (13, 1_600_000, 1_500_000, True),
                                              (14, 2_200_000, 1_000_000, True)])
def test_records_graph_vs_oracle(seed, n, nf, paired):
    rec = engine.synth_records(seed, n, 0, nf, paired)
    check_records(rec, n)


def test_records_unsorted_and_detection():
    rec = engine.synth_records(8, 5000, 0, 100_000, True)
    rng = np.random.default_rng(0)
    shuf = rec[rng.permutation(len(rec))]
    e1 = check_records(shuf, 5000, grouped=False)
    e2 = engine.graph_from_records(rec, 5000, grouped=True)
    assert np.array_equal(e1.weight, e2.weight)
    with pytest.raises(_lib.KarmaError) as ei:
        engine.graph_from_records(shuf, 5000, grouped=True)
    assert ei.value.code == _lib.KARMA_ERR_UNSORTED


def test_records_bucket_overflow_path():
    # every read hits 8 random contigs of 1000 -> > 3072 distinct pairs per bucket
    rng = np.random.default_rng(1)
    R = 60_000
    reads = np.repeat(np.arange(R, dtype=np.uint32), 8)
    contigs = rng.integers(0, 1000, R * 8).astype(np.uint32)
    check_records(np.stack([reads, contigs], 1), 1000)


def test_records_overflow_with_compact_reads():
    # a bucket that overflows its hash table also holds compact reads (span < 4):
    # the generic fallback must regenerate their pairs from the code histogram
    rng = np.random.default_rng(5)
    rows = []
    for r in range(40_000):
        if r % 2:
            for c in rng.integers(0, 1000, 8):
                rows.append((r, int(c)))
        else:
            m0 = int(rng.integers(0, 996))
            for c in m0 + rng.integers(0, 4, int(rng.integers(1, 6))):
                rows.append((r, int(c)))
    check_records(np.array(rows, np.uint32), 1000)


def test_records_compact_spans_and_bucket_edges():
    # spans 0..5 placed on and across pair-bucket boundaries (16 contigs per
    # bucket at n_contigs = 300): compact codes, bucket-crossing and wide reads
    rng = np.random.default_rng(6)
    rows = []
    for r in range(30_000):
        span = int(rng.integers(0, 6))
        m0 = int(rng.choice([15, 16, 30, 31, 32, 47, 100, 294])) - int(rng.integers(0, 3))
        cs = [m0, min(m0 + span, 299)] + [m0 + int(x) for x in rng.integers(0, span + 1, int(rng.integers(0, 4)))]
        for c in rng.permutation(cs):
            rows.append((r, min(int(c), 299)))
    check_records(np.array(rows, np.uint32), 300)


@pytest.mark.parametrize("n", [200, 1_200_000, 2_500_000])  # 2.5M: the 64-bit-key path (n_contigs > 2^21)
def test_records_big_reads_and_duplicates(n):
    rng = np.random.default_rng(2)
    rows = []
    for r in range(3000):
        m = int(rng.choice([1, 2, 3, 9, 17, 40]))
        lo = int(rng.integers(0, n - 200)) if n > 200 else 0
        for c in rng.integers(lo, lo + 200, m):
            rows.append((r, int(c)))
            if rng.random() < 0.3:
                rows.append((r, int(c)))  # mate on the same contig
    check_records(np.array(rows, np.uint32), n)


@pytest.mark.parametrize("n,nf", [(20_000, 400_000), (600_000, 1_000_000)])
def test_records_shuffled_contig_ids_relabel(n, nf):
    """Contig ids without isoform adjacency: most reads leave the compact path,
    so the job relabels the contigs (graph_sets.hip relabel_gate_kernel) and
    reruns on the new ids; reads of > 8 records and a contig-id shuffle of the
    same records must give the oracle's result on the original ids."""
    rec = np.ascontiguousarray(engine.synth_records(21, n, 0, nf, True))
    perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
    rec[:, 1] = perm[rec[:, 1]]
    rng = np.random.default_rng(4)
    r0 = int(rec[-1, 0]) + 1
    big = [(r0 + r, int(c)) for r in range(300) for c in rng.integers(0, n, int(rng.choice([9, 12, 30])))]
    check_records(np.concatenate([rec, np.array(big, np.uint32)]), n)


def test_records_empty_and_bad_contig():
    e = engine.graph_from_records(np.zeros((0, 2), np.uint32), 10)
    assert len(e.a) == 0 and e.totals.tolist() == [0] * 10
    with pytest.raises(_lib.KarmaError):
        engine.graph_from_records(np.array([[0, 12]], np.uint32), 10)
    e = engine.graph_from_records(np.zeros(0, np.uint32), 10, flagged=True)
    assert len(e.a) == 0 and e.totals.tolist() == [0] * 10
    with pytest.raises(_lib.KarmaError):
        engine.graph_from_records(engine.flag_records(np.array([[0, 12]], np.uint32)), 10, flagged=True)


def test_flagged_records_first_flag_and_chunk_edges():
    """KARMA_REC_FLAGGED edge cases: record 0 without its start flag still
    starts the first read; reads of 1..12 records placed across the 8,192- and
    4,096-record chunk edges and the 512-record steps' lane edges (the carried
    tail, the chunk-end walk, big reads at an edge); a device pointer that is
    not 16-byte aligned (the library copies it)."""
    rng = np.random.default_rng(17)
    rows, r = [], 0
    while len(rows) < 60_000:
        near = len(rows) % 4096 > 4080 or len(rows) % 512 > 500
        m = int(rng.choice([1, 2, 3, 5, 8, 9, 12])) if near else int(rng.integers(1, 5))
        m0 = int(rng.integers(0, 2996))
        for c in m0 + rng.integers(0, 5, m):
            rows.append((r, int(c)))
        r += 1
    rec = np.array(rows, np.uint32)
    check_records(rec, 3000)
    w = engine.flag_records(rec)
    w[0] &= np.uint32(0x7FFFFFFF)  # record 0 starts a read whatever its flag
    e = engine.graph_from_records(w, 3000, flagged=True)
    ref = engine.graph_from_records(rec, 3000)
    assert np.array_equal(e.a, ref.a) and np.array_equal(e.weight.view(np.uint64), ref.weight.view(np.uint64))
    ctx = _lib.default_context()
    buf = _lib.DevBuf(ctx, (len(w) + 1,), np.uint32)
    buf.view(1, len(w)).copy_from(w)
    p = engine.Pairs.from_records(ctx, None, 3000, device_ptr=buf.ptr + 4, n_records=len(w), flagged=True)
    q = engine.Pairs.from_records(ctx, rec, 3000)
    try:
        k, c, _ = p.get()
        k2, c2, _ = q.get()
        assert np.array_equal(k, k2) and np.array_equal(c, c2)
    finally:
        p.close()
        q.close()
        buf.close()


def test_records_compact_reads_of_9_to_16_at_chunk_edges():
    """Compact reads of 9, 12 and 16 records ending at, straddling and starting
    at every multiple of 4,096 records (tests/record_layouts.py; the deferred
    step's view of it: test_gpu_step.py), in both record formats."""
    rec, _ = chunk_edge_records()
    check_records(rec, 3000)


@pytest.mark.parametrize("n", [3000, 1_200_000, 2_200_000])  # binned, compact unbinned, no compact path
def test_flagged_records_sixteen_per_lane(n):
    """Flagged classify steps hold 16 records per lane (graph_sets.hip
    classify2_kernel's RPL): reads of 9..16 records inside one lane (compact: a code;
    general: the big list, as the general path reads 8), a read filling a lane
    exactly (a tail seen whole), reads of 17..40 records (lanes without a
    start), and runs of one-record reads (1,024 codes per step: the staging
    buffer's mid-walk flush), each compact and wide."""
    rng = np.random.default_rng(23)
    rows, r = [], 0

    def read(m, compact):
        nonlocal r
        lo = int(rng.integers(0, n - 200))
        cs = lo + (rng.integers(0, 4, m) if compact else rng.integers(0, 200, m))
        rows.extend((r, int(c)) for c in cs)
        r += 1

    def align(k):  # one-record reads up to a multiple of k records
        while len(rows) % k:
            read(1, True)

    while len(rows) < 120_000:
        kind = int(rng.integers(0, 5))
        if kind == 0:
            align(16)
            for _ in range(int(rng.integers(1, 40))):
                read(16, bool(rng.random() < 0.6))
        elif kind == 1:
            for _ in range(int(rng.integers(1, 2048))):
                read(1, bool(rng.random() < 0.9))
        elif kind == 2:
            read(int(rng.integers(17, 41)), bool(rng.random() < 0.5))
        else:
            if rng.random() < 0.5:
                align(16)
                read(int(rng.integers(1, 8)), True)
            read(int(rng.integers(9, 17)), bool(rng.random() < 0.5))
    check_records(np.array(rows, np.uint32), n)


@pytest.mark.parametrize("pos", [0, 1023, 1024, 2047, 4095, 8191, 12_345])
def test_records_contig_range_per_read_kind(pos):
    """The binned flagged classify checks the contig range per code (a compact
    code with m0 >= N - 3 sends its step to the replay, which checks the
    step's codes exactly) and leaves general and big reads to the kernels that
    read their records (graph_sets.hip RC).  A read with a contig >= N placed
    at `pos` (lane, 1,024-record step and 4,096 / 8,192-record chunk edges) as
    a compact read near N, a wide (general) read and a big read must fail in
    both record formats; the same reads with every contig < N must match the
    oracle."""
    n = 3000
    rng = np.random.default_rng(pos + 1)

    def build(read):
        rows = [(r, int(c)) for r, c in enumerate(rng.integers(0, n - 40, pos))]
        r = pos
        rows += [(r, c) for c in read]
        rest = rng.integers(0, n - 40, 30_000)
        rows += [(r + 1 + i, int(c)) for i, c in enumerate(rest)]
        return np.array(rows, np.uint32)

    # (ids >= 2^28: the staged code's m0 << 4 would wrap them onto small ids)
    bad_reads = [[n - 2, n], [n - 1, n + 2, n - 1], [5, 900, n + 7], [10 + i for i in range(11)] + [n],
                 [n + 100], [n - 3, n - 3, n - 1, n - 2, n + 1], [(1 << 28) + 5], [(1 << 28) + 5, (1 << 28) + 7],
                 [(1 << 30) + 2, (1 << 30) + 2], [(1 << 31) - 1], [7, (1 << 29) + 8]]
    for read in bad_reads:
        rec = build(read)
        for flagged in (False, True):
            x = engine.flag_records(rec) if flagged else rec
            with pytest.raises(_lib.KarmaError):
                engine.graph_from_records(x, n, flagged=flagged)
    for read in ([n - 2, n - 1], [n - 4, n - 1, n - 2], [n - 1], [5, 900, n - 1], [10 + i for i in range(11)] + [n - 1]):
        check_records(build(read), n)


def test_eq_vs_oracle_seeded():
    classes = synth.eq_classes(31, 2000, 300_000, True)
    names = [f"ctg{i}" for i in range(2000)]
    off = np.r_[0, np.cumsum([len(c) for c, _ in classes])].astype(np.int64)
    mem = np.array([x for c, _ in classes for x in c], np.uint32)
    cnt = np.array([k for _, k in classes], np.int64)
    skip = np.array([1 if len(c) == 1 else 0 for c, _ in classes], np.uint8)
    e = engine.graph_from_eq(off, mem, cnt, skip, len(names))
    o = oracle.graph_groups(off, mem, cnt, skip, len(names), dedup=False)
    for k in ("a", "b", "shared", "first", "totals"):
        assert np.array_equal(getattr(e, k), o[k]), k
    assert np.array_equal(e.weight.view(np.uint64), o["weight"].view(np.uint64))


@pytest.mark.parametrize("hub", [0, 9000])
def test_eq_ordered_edges_are_the_insertion_order(hub):
    """karma_edges_get_ordered: (a, b, w) grouped by a, inside a group by the
    pair's first emission -- the order read_graph.py:96-131 inserts edges in
    (the drop-in builds its graph from it).  Against the oracle's (a, first)
    order; hub > 0 adds a contig paired with `hub` others in shuffled class
    order (one run longer than the kernel's 4,096-entry LDS chunk)."""
    rng = np.random.default_rng(5 + hub)
    n = 12_000
    classes = synth.eq_classes(33, n, 200_000, True)
    cl = [np.asarray(c, np.uint32) for c, _ in classes]
    cn = [k for _, k in classes]
    if hub:
        for v in rng.permutation(np.arange(1, hub + 1)):
            cl.append(np.array([0, v], np.uint32))
            cn.append(int(rng.integers(1, 9)))
    off = np.r_[0, np.cumsum([len(c) for c in cl])].astype(np.int64)
    mem = np.concatenate(cl).astype(np.uint32)
    cnt = np.asarray(cn, np.int64)
    skip = np.array([1 if len(c) == 1 else 0 for c in cl], np.uint8)
    a, b, w = engine.graph_from_eq_ordered(off, mem, cnt, skip, n)
    o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
    order = np.lexsort((o["first"], o["a"]))
    assert np.array_equal(a, o["a"][order]) and np.array_equal(b, o["b"][order])
    assert np.array_equal(w.view(np.uint64), o["weight"][order].view(np.uint64))
    if hub:
        assert int(np.sum(a == 0)) >= hub


def test_eq_compact_inputs_match_wide():
    """karma_graph_eq_compact (sizes u8 with the size token "1" in bit 7, u32
    counts; offsets and skip flags rebuilt on the device by one scan) against
    the oracle: classes up to 127 members, token-"1" classes of several
    members, counts near 2^32, an empty class list; a member out of range
    fails it as on the wide path."""
    rng = np.random.default_rng(41)
    n = 2500
    cl = [rng.integers(0, n, int(m)).astype(np.uint32) for m in list(rng.integers(1, 6, 4000)) + [127, 90, 2, 1]]
    off = np.r_[0, np.cumsum([len(c) for c in cl])].astype(np.int64)
    mem = np.concatenate(cl).astype(np.uint32)
    cnt = rng.integers(1, 2**32 - 1, len(cl)).astype(np.int64)
    skip = (rng.random(len(cl)) < 0.05).astype(np.uint8)
    skip[-4] = 1  # the 127-member class with size token "1"
    sz, c32 = engine.eq_compact(off, cnt, skip)
    a, b, w = engine.graph_from_eq_compact_ordered(sz, mem, c32, n)
    o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
    order = np.lexsort((o["first"], o["a"]))
    assert np.array_equal(a, o["a"][order]) and np.array_equal(b, o["b"][order])
    assert np.array_equal(w.view(np.uint64), o["weight"][order].view(np.uint64))
    a0, _, _ = engine.graph_from_eq_compact_ordered(np.zeros(0, np.uint8), np.zeros(0, np.uint32),
                                                    np.zeros(0, np.uint32), n)
    assert len(a0) == 0
    m2 = mem.copy()
    m2[int(off[7])] = n + 1
    with pytest.raises(_lib.KarmaError) as ei:
        engine.graph_from_eq_compact_ordered(sz, m2, c32, n)
    assert ei.value.code == _lib.KARMA_ERR_ARG, str(ei.value)
    # sizes that disagree with the members' length: an error, no read past them
    for short in (mem[:-5], mem[:10]):
        with pytest.raises(_lib.KarmaError) as ei:
            engine.graph_from_eq_compact_ordered(sz, short, c32, n)
        assert ei.value.code == _lib.KARMA_ERR_ARG and "disagree" in str(ei.value), str(ei.value)
    one = np.array([1, 1, 1], np.uint8)  # three single-member classes, two members given (no pairs)
    with pytest.raises(_lib.KarmaError) as ei:
        engine.graph_from_eq_compact_ordered(one, np.array([3, 4], np.uint32), np.ones(3, np.uint32), n)
    assert "disagree" in str(ei.value), str(ei.value)
    a, _, _ = engine.graph_from_eq_compact_ordered(sz, mem, c32, n)  # the context still works
    assert len(a) > 0


def test_eq_big_classes_device_inputs_and_errors():
    """Classes past the per-thread size (a block each in eq_rank), duplicate
    members, size-token-"1" classes of several members, the skip array absent,
    and the inputs already on the device (karma_graph_eq is_device = 1):
    bit-exact against the oracle; a member id >= n_contigs fails the call on
    both paths, in a pair or alone in its class."""
    rng = np.random.default_rng(77)
    n = 1500
    sizes = list(rng.integers(1, 5, 3000)) + [33, 40, 100, 600, 2]
    classes = []
    for m in sizes:
        mem = rng.integers(0, n, int(m)) if m < 100 else np.r_[rng.integers(0, n, int(m) - 3), [5, 5, 5]]
        classes.append(np.asarray(mem, np.uint32))
    off = np.r_[0, np.cumsum([len(c) for c in classes])].astype(np.int64)
    mem = np.concatenate(classes).astype(np.uint32)
    cnt = rng.integers(1, 50, len(classes)).astype(np.int64)
    skip = (rng.random(len(classes)) < 0.05).astype(np.uint8)
    skip[-3] = 1  # a 100-member class with size token "1"
    for sk in (skip, None):
        e = engine.graph_from_eq(off, mem, cnt, sk if sk is not None else np.zeros(0, np.uint8), n) \
            if sk is not None else None
        o = oracle.graph_groups(off, mem, cnt, sk, n, dedup=False)
        if e is None:  # no skip array: through the C ABI with NULL
            ctx = _lib.default_context()
            h = ctypes.c_void_p()
            _lib.call("karma_graph_eq", ctx.h, _lib.ptr(off), _lib.ptr(mem), _lib.ptr(cnt), None, len(classes), n, 0,
                      ctypes.byref(h))
            p = engine.Pairs(ctx, h)
            ed = p.edges(_lib.KARMA_MODE_EQ, n)
            e = ed.get()
            ed.close()
            p.close()
        for k in ("a", "b", "shared", "first", "totals"):
            assert np.array_equal(getattr(e, k), o[k]), k
        assert np.array_equal(e.weight.view(np.uint64), o["weight"].view(np.uint64))
    # the same from device arrays
    ctx = _lib.default_context()
    bufs = [_lib.DevBuf.from_numpy(ctx, x) for x in (off, mem, cnt, skip)]
    try:
        h = ctypes.c_void_p()
        _lib.call("karma_graph_eq", ctx.h, *(ctypes.c_void_p(b.ptr) for b in bufs), len(classes), n, 1,
                  ctypes.byref(h))
        p = engine.Pairs(ctx, h)
        ed = p.edges(_lib.KARMA_MODE_EQ, n)
        e = ed.get()
        ed.close()
        p.close()
        o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
        for k in ("a", "b", "shared", "first", "totals"):
            assert np.array_equal(getattr(e, k), o[k]), k
    finally:
        for b in bufs:
            b.close()
    # out-of-range members: the argument error, and no kernel touches memory
    # out of bounds on the way (the context stays usable)
    for bad_at in (int(off[10]), int(off[-1]) - 1):  # inside a pair / the last class
        m2 = mem.copy()
        m2[bad_at] = n + 3
        with pytest.raises(_lib.KarmaError) as ei:
            engine.graph_from_eq(off, m2, cnt, skip, n)
        assert ei.value.code == _lib.KARMA_ERR_ARG, str(ei.value)
    one = np.array([0, 1], np.int64)
    with pytest.raises(_lib.KarmaError) as ei:  # a lone member out of range
        engine.graph_from_eq(one, np.array([n], np.uint32), np.array([3], np.int64), np.zeros(1, np.uint8), n)
    assert ei.value.code == _lib.KARMA_ERR_ARG, str(ei.value)
    e = engine.graph_from_eq(off, mem, cnt, skip, n)  # the context still works
    assert len(e.a) > 0


def test_eq_speculative_capacity_grows_and_shrinks():
    """karma_graph_eq sizes its pair scratch from the context's previous pair
    total (no readback): a call with more pairs than that runs again, sized;
    one with fewer uses the larger scratch.  Both bit-exact."""
    ctx = _lib.Context(0)
    try:
        for seed, n, nf in ((5, 300, 3000), (6, 3000, 200_000), (7, 200, 1000), (8, 4000, 300_000)):
            classes = synth.eq_classes(seed, n, nf, True)
            off = np.r_[0, np.cumsum([len(c) for c, _ in classes])].astype(np.int64)
            mem = np.array([x for c, _ in classes for x in c], np.uint32)
            cnt = np.array([k for _, k in classes], np.int64)
            skip = np.array([1 if len(c) == 1 else 0 for c, _ in classes], np.uint8)
            e = engine.graph_from_eq(off, mem, cnt, skip, n, ctx=ctx)
            o = oracle.graph_groups(off, mem, cnt, skip, n, dedup=False)
            for k in ("a", "b", "shared", "first", "totals"):
                assert np.array_equal(getattr(e, k), o[k]), (seed, k)
            assert np.array_equal(e.weight.view(np.uint64), o["weight"].view(np.uint64))
    finally:
        ctx.close()


def test_eq_path_equals_readset_path():
    # eq-class graph == per-read graph when each fragment's dedup
    # set is its class
    seed, n, nf = 12, 4000, 200_000
    rec = engine.synth_records(seed, n, 0, nf, True)
    er = engine.graph_from_records(rec, n)
    classes = synth.eq_classes(seed, n, nf, True)
    off = np.r_[0, np.cumsum([len(c) for c, _ in classes])].astype(np.int64)
    mem = np.array([x for c, _ in classes for x in c], np.uint32)
    cnt = np.array([k for _, k in classes], np.int64)
    skip = np.array([1 if len(c) == 1 else 0 for c, _ in classes], np.uint8)
    ee = engine.graph_from_eq(off, mem, cnt, skip, n)
    assert np.array_equal(er.a, ee.a) and np.array_equal(er.b, ee.b)
    assert np.array_equal(er.weight.view(np.uint64), ee.weight.view(np.uint64))
    assert np.array_equal(er.totals, ee.totals)


@pytest.mark.parametrize("kmer,n_rate", [("5p6", 700), (3, 300), (7, 0), (6, 2000), (8, 0), (8, 250)])
def test_profile_presence_two_phase(kmer, n_rate):
    # > 4096 contigs: phase B of the presence pass runs (saturated or not),
    # exception k-mers appear only in late contigs for the high n_rate cases;
    # at k = 8 the first 4,096 contigs miss some of the 65,536 8-mers, so phase
    # B's blocks start unsaturated and the late ones may see the set completed
    # by the early ones' flushes (each block decides for its own contigs)
    n = 6000
    blob, offs, key_len = engine.synth_contigs(900 + n_rate, n, 40, 200, n_rate)
    seqs = OrderedDict((f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(n))
    prof, cols, tot = engine.kmer_profile(seqs, kmer)
    oprof, ocols, ocounts = oracle.calc_kmer_profile(seqs, kmer)
    assert cols == ocols
    assert np.array_equal(prof.view(np.uint64), oprof.view(np.uint64))
    assert np.array_equal(tot, ocounts.sum(axis=1))


@pytest.mark.parametrize("seed,n_runs,n", [(61, 8, 2_000_000), (62, 3, 5000), (63, 1, 17), (64, 5, 0),
                                           (65, 2, 1),
                                           # past 64 runs: ranking merges of 64-run groups, level by level
                                           (66, 100, 300_000), (67, 300, 40_000), (68, 65, 65)])
def test_merge_runs_and_split(seed, n_runs, n):
    # the exchange owner's merge of sorted per-sender slices
    # (karma_pairs_merge_runs: merge tree + sum of equal keys) equals numpy and
    # the generic sort-reduce; split finds rank boundaries on the device
    rng = np.random.default_rng(seed)
    n_contigs = 1_600_000
    cuts = np.sort(rng.integers(0, n + 1, n_runs - 1))
    lens = np.diff(np.r_[0, cuts, n]).astype(np.int64)
    a = rng.integers(200_000, 400_000, n, dtype=np.uint64)
    b = rng.integers(0, n_contigs, n, dtype=np.uint64)
    keys = (a << np.uint64(32)) | b
    keys[: n // 4] = keys[n // 2: n // 2 + n // 4]  # equal keys, in several runs
    off = np.r_[0, np.cumsum(lens)]
    for r in range(n_runs):  # each sender's slice is sorted; it may repeat a key
        keys[off[r]:off[r + 1]] = np.sort(keys[off[r]:off[r + 1]])
    counts = rng.integers(1, 1 << 40, n, dtype=np.int64)
    ctx = _lib.default_context()
    u, inv = np.unique(keys, return_inverse=True)
    c = np.zeros(len(u), np.int64)
    np.add.at(c, inv, counts)
    for runs in (lens.tolist(), None):
        p = engine.Pairs.merge(ctx, keys, counts, runs=runs)
        k2, c2, _ = p.get()
        assert np.array_equal(k2, u) and np.array_equal(c2, c)
        bounds = [0, 200_000, 300_000, 400_000, n_contigs]
        assert np.array_equal(p.split(bounds), np.searchsorted(u, np.array(bounds, np.uint64) << np.uint64(32)))
        p.close()
    # the exchange's wire format: interleaved (key, count) pairs in device memory
    import ctypes
    kc = np.stack([keys.view(np.int64), counts], 1).copy()
    dev = ctypes.c_void_p()
    _lib.call("karma_dev_alloc", ctx.h, max(16, kc.nbytes), ctypes.byref(dev))
    try:
        if n:
            _lib.call("karma_memcpy", ctx.h, dev, _lib.ptr(kc), kc.nbytes, 0)
        p = engine.Pairs.merge_runs_kc(ctx, dev.value if n else None, lens.tolist())
        k3, c3, _ = p.get()
        assert np.array_equal(k3, u) and np.array_equal(c3, c)
        p.get_kc(dev.value if len(u) else None)  # and back out in the same format
        back = np.zeros((len(u), 2), np.int64)
        if len(u):
            _lib.call("karma_memcpy", ctx.h, _lib.ptr(back), dev, back.nbytes, 1)
        assert np.array_equal(back[:, 0].view(np.uint64), u) and np.array_equal(back[:, 1], c)
        p.close()
    finally:
        _lib.load().karma_dev_free(ctx.h, dev)
    if n > 1 and lens.max() > 1:
        r = int(np.argmax(lens))
        bad = keys.copy()
        bad[off[r]], bad[off[r] + 1] = keys[off[r] + 1] + np.uint64(1), keys[off[r]]  # a descent inside a run
        with pytest.raises(_lib.KarmaError):
            engine.Pairs.merge(ctx, bad, counts, runs=lens.tolist())
        # the device wire-format merge checks order at its next synchronisation:
        # the accessor's compaction, or the edge stage (which sums the groups itself)
        kcb = np.stack([bad.view(np.int64), counts], 1).copy()
        dev = ctypes.c_void_p()
        _lib.call("karma_dev_alloc", ctx.h, kcb.nbytes, ctypes.byref(dev))
        try:
            _lib.call("karma_memcpy", ctx.h, dev, _lib.ptr(kcb), kcb.nbytes, 0)
            if n_runs > 64:  # past 64 runs the level-by-level merge checks at once
                with pytest.raises(_lib.KarmaError) as ei:
                    engine.Pairs.merge_runs_kc(ctx, dev.value, lens.tolist())
                assert ei.value.code == _lib.KARMA_ERR_UNSORTED
            for use in (("get", "edges", "edges_deferred") if n_runs <= 64 else ()):
                p = engine.Pairs.merge_runs_kc(ctx, dev.value, lens.tolist())
                with pytest.raises(_lib.KarmaError) as ei:
                    if use == "get":
                        p.get()
                    elif use == "edges":
                        e, _ = p.edges_begin(_lib.KARMA_MODE_READS, n_contigs)
                        e.end()
                    else:  # end without the count: the error comes with the first read
                        e, _ = p.edges_begin(_lib.KARMA_MODE_READS, n_contigs)
                        e.end(count=False)
                        e.E
                assert ei.value.code == _lib.KARMA_ERR_UNSORTED
                p.close()
        finally:
            _lib.load().karma_dev_free(ctx.h, dev)


def test_edges_of_unsummed_merge_equal_compacted():
    # a merged list with equal keys left adjacent (merge_runs_kc) gives the
    # same edges and totals as its compacted form, in one call or two halves
    import ctypes
    rng = np.random.default_rng(77)
    n_contigs, W = 3000, 5
    runs = []
    for _ in range(W):
        a = rng.integers(0, n_contigs, 40_000, dtype=np.uint64)
        b = np.minimum(a + rng.integers(0, 6, 40_000, dtype=np.uint64), n_contigs - 1)
        u = np.unique((a << np.uint64(32)) | b)
        runs.append(np.stack([u.view(np.int64), rng.integers(1, 50, len(u))], 1))
    kc = np.concatenate(runs).copy()
    ctx = _lib.default_context()
    dev = ctypes.c_void_p()
    _lib.call("karma_dev_alloc", ctx.h, kc.nbytes, ctypes.byref(dev))
    try:
        _lib.call("karma_memcpy", ctx.h, dev, _lib.ptr(kc), kc.nbytes, 0)
        lens = [len(r) for r in runs]
        p1 = engine.Pairs.merge_runs_kc(ctx, dev.value, lens)
        e1, _ = p1.edges_begin(_lib.KARMA_MODE_READS, n_contigs)
        g1 = e1.end().get()
        # the same with the count deferred to the first read
        p3 = engine.Pairs.merge_runs_kc(ctx, dev.value, lens)
        e3, _ = p3.edges_begin(_lib.KARMA_MODE_READS, n_contigs)
        e3.end(count=False)
        g3 = e3.get()
        assert e3.E == e1.E == len(g3.a)
        for f in ("a", "b", "shared", "totals"):
            assert np.array_equal(getattr(g1, f), getattr(g3, f)), f
        assert np.array_equal(g1.weight.view(np.uint64), g3.weight.view(np.uint64))
        p2 = engine.Pairs.merge_runs_kc(ctx, dev.value, lens)
        assert p2.count() < len(kc)  # compacted: the equal keys were summed
        g2 = p2.edges(_lib.KARMA_MODE_READS, n_contigs).get()
        for f in ("a", "b", "shared", "totals"):
            assert np.array_equal(getattr(g1, f), getattr(g2, f)), f
        assert np.array_equal(g1.weight.view(np.uint64), g2.weight.view(np.uint64))
        assert len(g1.a) > 1000
    finally:
        _lib.load().karma_dev_free(ctx.h, dev)


def test_graph_records_split_call():
    # karma_graph_records_begin/_end: same list as the one-call form; one open
    # job per context (a second begin raises), and _end consumes the job
    import ctypes
    rng = np.random.default_rng(71)
    n, A = 3000, 200_000
    rid = np.sort(rng.integers(0, A // 3, A)).astype(np.uint32)
    cid = rng.integers(0, n, A).astype(np.uint32)
    rec = np.stack([rid, cid], 1)
    ctx = _lib.default_context()
    ref = engine.Pairs.from_records(ctx, rec, n)
    k0, c0, _ = ref.get()
    dev = ctypes.c_void_p()  # device records through the library's own allocator
    _lib.call("karma_dev_alloc", ctx.h, rec.nbytes, ctypes.byref(dev))
    try:
        _lib.call("karma_memcpy", ctx.h, dev, _lib.ptr(rec), rec.nbytes, 0)
        job = engine.Pairs.from_records_begin(ctx, n, dev.value, A)
        with pytest.raises(_lib.KarmaError):
            engine.Pairs.from_records_begin(ctx, n, dev.value, A)
        p = job.end()
        k1, c1, _ = p.get()
        assert np.array_equal(k0, k1) and np.array_equal(c0, c1)
        job2 = engine.Pairs.from_records_begin(ctx, n, dev.value, A)  # the context is free again
        k2, c2, _ = job2.end().get()
        assert np.array_equal(k0, k2) and np.array_equal(c0, c2)
        # owner bounds given up front (karma_graph_split_hint): the final kernel's
        # starts equal a search of the finished list, also for bounds off the
        # bucket grid, at 0 and at n; other bounds still search
        for bounds in ([0, 1000, 2000, n], [0, 1, 1024, 1025, 2047, 2999, n], [0, n]):
            job3 = engine.Pairs.from_records_begin(ctx, n, dev.value, A, split_bounds=bounds)
            p3 = job3.end()
            want = np.searchsorted(k0, np.array(bounds, np.uint64) << np.uint64(32))
            assert np.array_equal(p3.split(bounds), want)
            assert np.array_equal(p3.split([0, 1500, n]), np.searchsorted(k0, np.array([0, 1500, n], np.uint64) << np.uint64(32)))
            p3.close()
    finally:
        _lib.load().karma_dev_free(ctx.h, dev)


@pytest.mark.parametrize("chunk", ["2048", "4096", "8192"])
def test_records_both_chunk_sizes(chunk, monkeypatch):
    """Classify's chunk size follows the launch size (graph_sets.hip
    chunk_records): inputs below ~134M records take 4096-record chunks, config
    3 and 5 take 8192.  KARMA_CHUNK pins either size so both run the small
    cases: reads across chunk boundaries, reads of > 8 records, a bucket
    overflow beside compact reads, and the relabelled rerun."""
    monkeypatch.setenv("KARMA_CHUNK", chunk)
    check_records(engine.synth_records(2, 20_000, 0, 400_000, True), 20_000)
    check_records(engine.synth_records(13, 1_600_000, 0, 1_500_000, True), 1_600_000)
    rng = np.random.default_rng(2)
    rows = []
    for r in range(3000):
        lo = int(rng.integers(0, 1000))
        for c in rng.integers(lo, lo + 200, int(rng.choice([1, 2, 3, 9, 17, 40]))):
            rows.append((r, int(c)))
    check_records(np.array(rows, np.uint32), 1200)
    rec = np.ascontiguousarray(engine.synth_records(21, 20_000, 0, 400_000, True))
    rec[:, 1] = np.random.default_rng(3).permutation(20_000).astype(np.uint32)[rec[:, 1]]
    check_records(rec, 20_000)


@pytest.mark.parametrize("binned", ["1", "0"])
def test_records_binned_classify_and_partition_paths(binned, monkeypatch):
    """The binned classify (codes straight into per-bucket segments, no code
    partition; graph_sets.hip classify2_kernel<.., BIN>, code_seg_reduce_kernel)
    and the partition path it replaces (KARMA_BIN=0) give the oracle's graph:
    a skewed input whose codes all fall in one bucket (dozens of back segments
    per chunk), the bucket-count limit of the binned path (56 code buckets at
    229,376 contigs; 57 takes the partition), reads across chunk boundaries at
    every chunk size, and the relabelled rerun."""
    monkeypatch.setenv("KARMA_BIN", binned)
    rng = np.random.default_rng(31)
    R = 120_000
    m0 = rng.integers(0, 4093, R)  # every compact code in code bucket 0
    span = rng.integers(0, 4, R)
    rows = np.stack([np.repeat(np.arange(R, dtype=np.uint32), 2),
                     np.stack([m0, m0 + span], 1).reshape(-1).astype(np.uint32)], 1)
    check_records(rows, 50_000)
    monkeypatch.setenv("KARMA_BACKLIST", "3")  # the code reduce's back-segment list overflows: full scan
    check_records(rows, 50_000)
    monkeypatch.delenv("KARMA_BACKLIST")
    for n in (229_376, 229_377):
        check_records(engine.synth_records(33, n, 0, 300_000, True), n)
    for chunk in ("2048", "8192"):
        monkeypatch.setenv("KARMA_CHUNK", chunk)
        check_records(engine.synth_records(34, 30_000, 0, 250_000, True), 30_000)
        check_records(rows, 50_000)
    monkeypatch.delenv("KARMA_CHUNK")
    rec = np.ascontiguousarray(engine.synth_records(21, 20_000, 0, 400_000, True))
    rec[:, 1] = np.random.default_rng(3).permutation(20_000).astype(np.uint32)[rec[:, 1]]
    check_records(rec, 20_000)
