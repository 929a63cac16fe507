"""The native step (karma_step, csrc/step.hip) against the oracle.

karma_amd/distributed.py ShardedBuild drives the library's karma_step for the
production path (one GPU, an emulated rank, RCCL ranks).  Its deferred steps
(outputs not read: count=False) wait for nothing: M, the records job's control
block and the tail's sizes stay on the device, a status kernel reports the
checks through mapped memory, and a step whose checks call for the general
path (relabelled contigs, bucket overflow, reads of > 8 records) runs again
synchronously.  Here: deferred steps, then sync, then the profile of the
newest deferred step and a kept step -- all bit-exact against the oracle --
and the slow paths and errors seen through the deferred checks."""
from collections import OrderedDict

import numpy as np
import pytest

from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import ShardedBuild
from oracle import oracle
from record_layouts import chunk_edge_records

pytestmark = pytest.mark.gpu

SEED = 41


def contigs(n, c_lo=0, n_rate=300):
    blob, offs, key_len = engine.synth_contigs(SEED, n, 30, 900, n_rate, first=c_lo)
    return blob, offs, key_len


def oracle_graph(rec, n):
    rs = np.asarray(rec, np.int64)
    st = np.flatnonzero(np.r_[True, rs[1:, 0] != rs[:-1, 0]]) if len(rs) else np.zeros(0, np.int64)
    return oracle.graph_groups(np.r_[st, len(rs)], rs[:, 1] if len(rs) else np.zeros(0), None, None, n, dedup=True)


def oracle_profile(blob, offs, c_lo, n):
    seqs = OrderedDict((f">ctg{c_lo + i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(n))
    prof, cols, _ = oracle.calc_kmer_profile(seqs, "5p6")
    return prof, cols


class Run:
    def __init__(self, n_glob, rec, emulate=1, n_rate=300, flagged=False):
        self.ctx = _lib.Context(0)
        self.n_glob = n_glob
        n_loc = n_glob // emulate if emulate > 1 else n_glob
        self.n_loc = n_loc
        self.blob, self.offs, kl = contigs(n_loc, n_rate=n_rate)
        self.build = ShardedBuild(self.ctx, SoloComm(), -1, n_glob, 0, n_loc, emulate_ranks=emulate,
                                  flagged=flagged)
        assert self.build.native is not None, "the native step drives the production path"
        self.store = engine.ContigStore(self.ctx, self.blob, self.offs, kl)
        self.rec = np.ascontiguousarray(rec)
        # the records as the step takes them: (read, contig) pairs or KARMA_REC_FLAGGED words
        self.dev = _lib.DevBuf.from_numpy(self.ctx, engine.flag_records(self.rec) if flagged
                                          else self.rec.view(np.int64).reshape(-1))

    def step(self, **kw):
        return self.build.run(self.store, self.dev.ptr, len(self.rec), **kw)

    def close(self):
        self.build.close()
        self.store.close()
        self.dev.close()
        self.ctx.close()


def check_edges(e, o):
    assert np.array_equal(e.a, o["a"]) and np.array_equal(e.b, o["b"])
    assert np.array_equal(e.shared, o["shared"])
    assert np.array_equal(e.weight.view(np.uint64), o["weight"].view(np.uint64))
    assert np.array_equal(e.totals, o["totals"])


@pytest.mark.parametrize("emulate,n_rate,flagged", [(1, 300, False), (3, 300, False), (1, 0, False), (8, 0, False),
                                                    (1, 300, True), (3, 0, True), (8, 300, True)])
def test_deferred_steps_then_kept_step_match_oracle(emulate, n_rate, flagged):
    n = 3000 if emulate == 1 else 3001  # 3001 / 3: owner bounds that do not divide evenly
    rec = engine.synth_records(SEED, n, 0, 300_000, True)
    r = Run(n, rec, emulate, n_rate, flagged)
    try:
        r.step(count=False)  # warm: allocations, events
        calls0 = _lib.api_calls()
        for _ in range(4):
            res = r.step(count=False)
            assert res["E_local"] is None
        calls = (_lib.api_calls() - calls0) / 4
        r.build.sync()
        info = r.build.native.info()
        # 5 deferred calls, then sync; nothing is slow, so no step runs again
        # and none runs synchronously.  Steps 1 and 2 are the first jobs of
        # the two main streams' tails (they size the tail's control block),
        # steps 3..5 take it: 3 on their own block.
        assert info[[4, 5, 6, 14]].tolist() == [0, 5, 0, 3], info.tolist()
        # the newest deferred step's profile (M read by the kernels on the device)
        prof_o, cols_o = oracle_profile(r.blob, r.offs, 0, r.n_loc)
        assert info[1] is not None
        got = r.build.native.profile().numpy()
        assert got.shape == prof_o.shape
        assert np.array_equal(got.view(np.uint64), prof_o.view(np.uint64))
        # ... and its edges, from the arrays the deferred tail kernels wrote
        # (step_edge_count / step_edge_write; emulated: step_merge_kernel first)
        o = oracle_graph(rec, n)
        e_def, deferred = r.build.native.newest_edges()
        assert deferred
        check_edges(e_def, o)
        assert int(info[1]) == len(o["a"]), (info.tolist(), len(o["a"]))
        # an ACGT-only store: a deferred step enqueues ~30 HIP calls and waits
        # for nothing (with non-ACGT bases the exception keys' count is read back)
        if n_rate == 0:
            assert calls <= 40, calls
        res = r.step(keep=True)
        assert engine.decode_keys(res["columns"], -1) == cols_o
        assert np.array_equal(res["profile"].numpy().view(np.uint64), prof_o.view(np.uint64))
        check_edges(res["edges"], o)
        assert res["E_local"] == len(res["edges"].a)
        # after sync, the newest deferred step's M and edge count (its status words)
        assert int(info[0]) == len(cols_o)
        assert int(info[1]) == len(res["edges"].a), (info.tolist(), len(res["edges"].a))
        # after a kept (synchronous) step the accessor answers with its edges
        e_sync, deferred = r.build.native.newest_edges()
        assert not deferred
        check_edges(e_sync, o)
    finally:
        r.close()


@pytest.mark.parametrize("big,flagged", [(True, False), (False, False), (True, True), (False, True)])
def test_deferred_steps_slow_path_runs_again(big, flagged):
    """Shuffled contig ids (most reads leave the compact path: the relabel vote)
    plus (big) reads of > 8 records: the deferred step's status calls for the
    general path and the step runs again synchronously; the next deferred steps
    run synchronously for a while; results stay exact.  Without big reads the
    relabel verdict alone calls for the rerun: on the step's own control block
    (from the second deferred step of each main stream) it comes from
    classify's chunk votes, not from the probe kernel."""
    n = 4000
    rec = np.ascontiguousarray(engine.synth_records(SEED, n, 0, 200_000, True))
    perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
    rec[:, 1] = perm[rec[:, 1]]
    if big:
        rng = np.random.default_rng(4)
        r0 = int(rec[-1, 0]) + 1
        extra = np.array([(r0 + i, int(c)) for i in range(200) for c in rng.integers(0, n, 12)], np.uint32)
        rec = np.concatenate([rec, extra])
    r = Run(n, rec, flagged=flagged)
    try:
        for _ in range(3 if big else 12):
            r.step(count=False)
        r.build.sync()
        info = r.build.native.info()
        if big:
            # 3 deferred calls (none reaches the lag point: 3 pending), then
            # sync reads all three: each is slow and runs again (3 synchronous
            # steps).  Step 3 is the second job of its tail: 1 own block.
            assert info[[4, 5, 6, 14]].tolist() == [3, 3, 3, 1], info.tolist()
        else:
            # calls 1..3 deferred; call 4 is the lag point of step 1 (waits for
            # it: slow, it runs again, sticky = 8) and still runs deferred; call
            # 5 is sticky: it checks steps 2..4 (all slow: 3 more re-runs) and
            # runs synchronously, as do calls 6..12.  4 deferred, 4 re-run,
            # 4 + 8 synchronous; steps 3 and 4 ran on their tail's own block,
            # so their verdicts came from classify's votes, not from the probe.
            assert info[[4, 5, 6, 14]].tolist() == [12, 4, 4, 2], info.tolist()
        res = r.step(keep=True)
        check_edges(res["edges"], oracle_graph(rec, n))
    finally:
        r.close()


def test_deferred_steps_on_own_control_block_launch_no_probe():
    """From the second deferred step of each main stream on, the records job
    takes the step's own zeroed control block: no relabel probe launch ahead of
    classify (the relabel verdict comes from classify's votes); results exact."""
    n = 3000
    rec = engine.synth_records(SEED, n, 0, 300_000, True)
    r = Run(n, rec)
    try:
        for _ in range(3):
            r.step(count=False)  # each main stream's first job sizes its control block
        r.build.sync()
        info0 = r.build.native.info()
        # steps 1 and 2 size their tails' blocks, step 3 takes its tail's
        assert info0[[4, 5, 6, 14]].tolist() == [0, 3, 0, 1], info0.tolist()
        own0 = int(info0[14])
        r.ctx.timing(True, "relabel_probe")
        r.ctx.timing_reset()
        for _ in range(6):
            r.step(count=False)
        r.build.sync()
        probes = r.ctx.timing_read().get("relabel_probe", (0.0, 0))[1]
        r.ctx.timing(False)
        info = r.build.native.info()
        assert int(info[14]) - own0 == 6, info
        assert probes == 0, probes
        # 3 + 6 deferred calls, nothing slow: none synchronous, none run again
        assert info[[4, 5, 6, 14]].tolist() == [0, 9, 0, 7], info.tolist()
        res = r.step(keep=True)
        check_edges(res["edges"], oracle_graph(rec, n))
    finally:
        r.close()


def test_deferred_step_bucket_overflow_runs_again():
    rng = np.random.default_rng(1)
    R = 60_000
    reads = np.repeat(np.arange(R, dtype=np.uint32), 8)
    cs = rng.integers(0, 1000, R * 8).astype(np.uint32)
    rec = np.stack([reads, cs], 1)
    r = Run(1000, rec)
    try:
        r.step(count=False)
        r.build.sync()
        # one deferred call (its tail's first job: not on an own block); sync
        # reads its status: slow, it runs again (the one synchronous step)
        info = r.build.native.info()
        assert info[[4, 5, 6, 14]].tolist() == [1, 1, 1, 0], info.tolist()
        res = r.step(keep=True)
        check_edges(res["edges"], oracle_graph(rec, 1000))
    finally:
        r.close()


def test_deferred_step_unsorted_records_error_reported():
    rec = engine.synth_records(SEED, 2000, 0, 50_000, True)
    shuf = rec[np.random.default_rng(0).permutation(len(rec))]
    r = Run(2000, shuf)
    try:
        r.step(count=False)  # returns at once; the error arrives with the deferred check
        with pytest.raises(_lib.KarmaError) as ei:
            r.build.sync()
        assert ei.value.code == _lib.KARMA_ERR_UNSORTED
    finally:
        r.close()


def test_native_step_equals_python_driver():
    """The native step and the Python driver (HipOps, kept for the host-staged
    rehearsal transport) give the same bytes, one GPU and an emulated rank."""
    from karma_amd.distributed import HipOps

    n = 2500
    rec = engine.synth_records(SEED + 1, n, 0, 150_000, True)
    for emulate in (1, 4):
        outs = []
        for python in (False, True):
            ctx = _lib.Context(0)
            n_loc = n // emulate
            blob, offs, kl = contigs(n_loc)
            b = ShardedBuild(ctx, SoloComm(), -1, n, 0, n_loc, ops=HipOps(ctx) if python else None,
                             emulate_ranks=emulate)
            assert (b.native is None) == python
            st = engine.ContigStore(ctx, blob, offs, kl)
            d = _lib.DevBuf.from_numpy(ctx, rec.view(np.int64).reshape(-1))
            res = b.run(st, d.ptr, len(rec), keep=True)
            e = res["edges"]
            outs.append([res["profile"].numpy(), np.asarray(res["columns"]), e.a, e.b, e.shared, e.weight, e.totals,
                         np.array([res["M"], res["E_local"], res["entries"], res["pairs_local"]])])
            b.close()
            st.close()
            d.close()
            ctx.close()
        for x, y in zip(*outs):
            assert x.shape == y.shape and np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def test_two_steps_on_one_context_keep_their_own_status():
    """Two live native steps on one context (two ShardedBuilds of different
    shapes) interleave deferred steps: each has its own mapped status ring, so
    neither reads the other's verdicts, and each one's newest profile, M and
    edge count are its own (csrc/step.hip karma_step::ring_mem)."""
    ctx = _lib.Context(0)
    objs = []
    try:
        runs = []
        for n, nf, seed in ((2000, 120_000, SEED), (3500, 200_000, SEED + 7)):
            blob, offs, kl = engine.synth_contigs(seed, n, 30, 900, 0)
            rec = np.ascontiguousarray(engine.synth_records(seed, n, 0, nf, True))
            b = ShardedBuild(ctx, SoloComm(), -1, n, 0, n)
            st = engine.ContigStore(ctx, blob, offs, kl)
            d = _lib.DevBuf.from_numpy(ctx, rec.view(np.int64).reshape(-1))
            objs += [b, st, d]
            runs.append((b, st, d, rec, n, blob, offs))
        for _ in range(4):
            for b, st, d, rec, *_ in runs:
                b.run(st, d.ptr, len(rec), count=False)
        for b, st, d, rec, n, blob, offs in runs:
            b.sync()
            info = b.native.info()
            # per step object: 4 deferred calls (the 4th waits for the 1st's
            # status at its lag point), then sync; nothing slow.  Steps 3 and
            # 4 are the second jobs of their tails: 2 on their own block.
            assert info[[4, 5, 6, 14]].tolist() == [0, 4, 0, 2], info.tolist()
            prof_o, cols_o = oracle_profile(blob, offs, 0, n)
            assert int(info[0]) == len(cols_o)
            assert int(info[1]) == len(oracle_graph(rec, n)["a"])
            got = b.native.profile().numpy()
            assert np.array_equal(got.view(np.uint64), prof_o.view(np.uint64))
    finally:
        for o in objs:
            o.close()
        ctx.close()


def test_middle_deferred_step_rerun_keeps_newest_outputs():
    """Three deferred steps of which the middle one holds reads of > 8 records
    (its status calls for the general path, so karma_step_sync runs it again
    synchronously): the newest step's M and edge count stay the ones reported
    after sync, not the re-run's."""
    n = 3000
    rec = np.ascontiguousarray(engine.synth_records(SEED, n, 0, 150_000, True))
    rng = np.random.default_rng(9)
    r0 = int(rec[-1, 0]) + 1
    big = np.array([(r0 + i, int(c)) for i in range(50) for c in rng.integers(0, n, 12)], np.uint32)
    rec_big = np.concatenate([rec, big])
    r = Run(n, rec, n_rate=0)
    d_big = _lib.DevBuf.from_numpy(r.ctx, rec_big.view(np.int64).reshape(-1))
    try:
        r.step(count=False)
        r.build.run(r.store, d_big.ptr, len(rec_big), count=False)
        r.step(count=False)
        r.build.sync()
        info = r.build.native.info()
        # 3 deferred calls, then sync reads all three: only the middle step is
        # slow and runs again (1 synchronous).  Step 3 is the second job of
        # step 1's tail, with the same records: 1 on its own block.
        assert info[[4, 5, 6, 14]].tolist() == [1, 3, 1, 1], info.tolist()
        e_new = len(oracle_graph(rec, n)["a"])
        assert len(oracle_graph(rec_big, n)["a"]) != e_new  # the big reads add edges
        assert int(info[1]) == e_new, (info.tolist(), e_new)
        prof_o, cols_o = oracle_profile(r.blob, r.offs, 0, n)
        assert int(info[0]) == len(cols_o)
        assert np.array_equal(r.build.native.profile().numpy().view(np.uint64), prof_o.view(np.uint64))
    finally:
        d_big.close()
        r.close()


@pytest.mark.parametrize("fault_seq", [4, 5])
def test_failed_deferred_step_leaves_control_block_zeroed(monkeypatch, fault_seq):
    """A deferred step that fails after its records job and tail kernels ran
    (KARMA_STEP_FAULT_SEQ: the error path before the status kernel, which is
    what clears the tail's own control block) must leave that block zeroed:
    the next deferred jobs on the same tail take it as such.  Later deferred
    steps' profile and edges stay bit-exact (ADVICE r05, step.hip FailGuard)."""
    monkeypatch.setenv("KARMA_STEP_FAULT_SEQ", str(fault_seq))
    n = 3000
    rec = engine.synth_records(SEED, n, 0, 200_000, True)
    r = Run(n, rec, n_rate=0)
    try:
        failed = 0
        for _ in range(fault_seq + 4):  # both main streams' tails run again after the failure
            try:
                r.step(count=False)
            except _lib.KarmaError as e:
                assert "injected fault" in str(e)
                failed += 1
        assert failed == 1
        r.build.sync()
        info = r.build.native.info()
        # fault_seq + 4 deferred calls (the failed one counted: it fails after
        # its records job), none slow: no stale flag asked for a re-run.  Every
        # step from the 3rd on, the failed one included, took its tail's block.
        assert info[[4, 5, 6, 14]].tolist() == [0, fault_seq + 4, 0, fault_seq + 2], info.tolist()
        o = oracle_graph(rec, n)
        e, deferred = r.build.native.newest_edges()
        assert deferred
        check_edges(e, o)
        prof_o, _ = oracle_profile(r.blob, r.offs, 0, n)
        assert np.array_equal(r.build.native.profile().numpy().view(np.uint64), prof_o.view(np.uint64))
    finally:
        r.close()


@pytest.mark.parametrize("sticky", [False, True])
@pytest.mark.parametrize("flagged", [False, True])
def test_misaligned_deferred_records_refused_before_any_state_change(flagged, sticky):
    """KARMA_STEP_DEFER records must be 16-byte aligned: a misaligned pointer
    is KARMA_ERR_ARG on entry, before any counter, sequence number or field of
    the shared context changes -- karma_step_info is unchanged, a records job
    on the same context and the next steps stay bit-exact.  sticky: the same
    call while deferred calls run synchronously after a re-run (where the
    synchronous path would have copied the pointer): acceptance does not
    depend on that hidden state."""
    n = 3000
    rec = np.ascontiguousarray(engine.synth_records(SEED, n, 0, 100_000, True))
    r = Run(n, rec, flagged=flagged)
    d_big = None
    try:
        if sticky:
            rng = np.random.default_rng(9)
            r0 = int(rec[-1, 0]) + 1
            big = np.array([(r0 + i, int(c)) for i in range(50) for c in rng.integers(0, n, 12)], np.uint32)
            rec_big = np.concatenate([rec, big])
            d_big = _lib.DevBuf.from_numpy(r.ctx, engine.flag_records(rec_big) if flagged
                                           else rec_big.view(np.int64).reshape(-1))
            r.build.run(r.store, d_big.ptr, len(rec_big), count=False)
            r.build.sync()  # reads the step's status: big reads, it runs again; the next 8 deferred calls are sticky
        for _ in range(3):
            r.step(count=False)
        info0 = r.build.native.info()
        # not sticky: 3 deferred calls, the third on its tail's own block.
        # sticky: 1 deferred call, re-run at sync (1 synchronous), then 3 sticky
        # calls run synchronously; no job on an own block.
        assert info0[[4, 5, 6, 14]].tolist() == ([4, 1, 1, 0] if sticky else [0, 3, 0, 1]), info0.tolist()
        with pytest.raises(_lib.KarmaError) as ei:
            r.build.run(r.store, r.dev.ptr + (4 if flagged else 8), len(rec) - 1, count=False)
        assert ei.value.code == _lib.KARMA_ERR_ARG
        assert np.array_equal(r.build.native.info(), info0), (r.build.native.info().tolist(), info0.tolist())
        # the step is alive and may have deferred steps in flight: a records
        # job on its context finds none of the step's scheduling state there
        o = oracle_graph(rec, n)
        check_edges(engine.graph_from_records(engine.flag_records(rec) if flagged else rec, n, ctx=r.ctx,
                                              flagged=flagged), o)
        for _ in range(3):
            r.step(count=False)
        r.build.sync()
        info = r.build.native.info()
        # not sticky: 3 more deferred calls, each on its tail's own block, none
        # slow.  sticky: 3 more sticky calls run synchronously.
        assert info[[4, 5, 6, 14]].tolist() == ([7, 1, 1, 0] if sticky else [0, 6, 0, 4]), info.tolist()
        e, deferred = r.build.native.newest_edges()
        assert deferred == (not sticky)
        check_edges(e, o)
        prof_o, _ = oracle_profile(r.blob, r.offs, 0, n)
        assert np.array_equal(r.build.native.profile().numpy().view(np.uint64), prof_o.view(np.uint64))
    finally:
        if d_big is not None:
            d_big.close()
        r.close()


@pytest.fixture(scope="module")
def edge_layout():
    rec, placed = chunk_edge_records()
    return rec, placed, oracle_graph(rec, 3000)


def test_chunk_edge_layout_places_every_read_kind(edge_layout):
    rec, placed, _ = edge_layout
    assert len(rec) == 40_000 and len(placed) == 9
    assert sorted((m, pos) for _, m, pos in placed) == sorted((m, pos) for m in (9, 12, 16) for pos in "abc")
    for i, (start, m, pos) in enumerate(placed):
        edge = 4096 * (i + 1)
        ids = rec[start:start + m, 0]
        assert (ids == ids[0]).all() and rec[start - 1, 0] != ids[0] and rec[start + m, 0] != ids[0]
        assert int(rec[start:start + m, 1].max()) - int(rec[start:start + m, 1].min()) <= 3  # compact
        past = start + m - edge
        assert {"a": past == 0, "b": 1 <= past <= 7, "c": past == m}[pos], (start, m, pos)


def test_flagged_compact_reads_at_chunk_edges_stay_deferred(edge_layout):
    """Flagged records hold 16 per lane, so a compact read of 9..16 records is
    a code inside a chunk; the same read ending at, straddling or starting at a
    chunk edge (classify's chunk-end tail walk) must be one too -- not a big
    read, which would send every deferred step through a synchronous re-run."""
    rec, _, o = edge_layout
    r = Run(3000, rec, flagged=True)
    try:
        for _ in range(3):
            r.step(count=False)
        r.build.sync()
        info = r.build.native.info()
        # 3 deferred calls, then sync; nothing slow; step 3 on its tail's own block
        assert info[[4, 5, 6, 14]].tolist() == [0, 3, 0, 1], info.tolist()
        e, deferred = r.build.native.newest_edges()
        assert deferred
        check_edges(e, o)
    finally:
        r.close()


def test_flagged_wide_read_at_chunk_edge_runs_again():
    """The positive control of the test above: the same layout with one edge
    read made wide (12 records over 200 contig ids: general and longer than 8
    records, a big read) does ask for the re-run; results stay exact."""
    rec, placed = chunk_edge_records(wide_edge=4)
    assert placed[4][1:] == (12, "b")
    r = Run(3000, rec, flagged=True)
    try:
        for _ in range(3):
            r.step(count=False)
        r.build.sync()
        info = r.build.native.info()
        # 3 deferred calls, then sync reads all three: each holds the big read
        # and runs again (3 synchronous steps); step 3 on its tail's own block
        assert info[6] >= 1, info.tolist()
        assert info[[4, 5, 6, 14]].tolist() == [3, 3, 3, 1], info.tolist()
        e, deferred = r.build.native.newest_edges()
        check_edges(e, oracle_graph(rec, 3000))
    finally:
        r.close()
