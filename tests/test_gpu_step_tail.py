"""The deferred step's tail kernels (step.hip: step_pack_kernel,
step_merge_kernel, step_edge_count_kernel, step_edge_write_kernel) against a
plain model, on record batches built (tests/step_tail_reference.py) to land on
those kernels' limits.

One process, emulated owners: NativeStep with hand-made owner bounds, this
process holding 16 contigs.  Several ranks: threads of one child process over
the RCCL test double (tests/fake_rccl_ranks.py --case tail), the merge reading
the all-to-all's slots.  Every case runs after two deferred dirtying steps on
the same step object (one per tail: each gives every contig a nonzero total,
every edge tile edges and a longer list), so totals, tile counts and the
merged list are read out of used buffers.  Every comparison is exact against
the model of the whole batch: a, b, shared, the weights' bits, the totals over
all n_glob, info()[1] == E.  Every case asserts that it stayed deferred (or,
slot_kc_plus_1 alone, that every rank ran the step again): a case that falls
back to the synchronous path would test graph.hip instead.

Which branch each case pins (wN: N emulated owners, w1: no merge):
  edge_len_U                     U = 0 (no records), 1, ET - 1, ET, ET + 1, 2 ET + 1
  edge_empty_tile, *_only        a tile without an edge between two with; every key diagonal (E = 0)
  edge_second_round              more edge tiles than the edge stage's grid (from the export): the second
                                 grid-stride round, its prefix over every tile of the first
  totals_past_*                  contigs before the first key, gaps of 1, 2 and 1,500, 1 / 2 / 5,003 contigs
                                 past the last key, n_glob odd
  weights                        repeated reads; >= 50 quotients a reciprocal multiply gets wrong.  (A count
                                 above 2^53, where int64 -> f64 rounds, cannot come from records.)
  ranks_2 / 8 / 9 / 64           MFAST, one over, MAX_RUNS owners; bounds on a bucket edge, inside a bucket,
                                 in the last bucket; ranks_8_flagged: KARMA_REC_FLAGGED records (a seam check)
  empty_owners                   empty owners first, in the middle, last; a bound at n_glob on a bucket edge
  owner_slices                   slices of MT - 1, MT, MT + 1 keys
  merge_stride                   more merge tiles than the merge's grid (from the export)
  ties_2 / 3 / 8, world_9        the same reads on every rank: <= before, < after; a group of W equal keys
                                 across elements ET - 1 | ET; nine runs: no tile on the lockstep path
  window_*                       a tile's window of 0, 1, 2, 3, 4, 2^j - 1, 2^j keys (j = 3..10); 1 beside
                                 5,000; MLDS - 1, MLDS, MLDS + 1 (that tile alone leaves the lockstep path);
                                 two that fit only alone; a spilled window, then a small staged one
  run_lengths                    slot headers 0, 1, MT - 1, MT, MT + 1; an owner that receives nothing
  run_touch                      runs that touch in one key at a tile edge inside a run: the before / after
                                 shortcut's <= and <
  slot_kc, slot_kc_plus_1        a slice of exactly the slot's room stays deferred; one more: every rank
                                 runs the step again

Strength check (done once, by hand; nothing of it is kept): seven copies of
the library, each with one comparison of step.hip changed so that every index
stays in bounds, each run once against this file.
  the lockstep path's tie rule          14 of 15 rank cases fail (run_lengths, slot_kc, ties_*, window_*:
  (sr < r ? m <= k : m < k) -> <        two equal keys on one slot, the stale slot gives a zero total);
                                        world_9 passes, as it must: nine runs never take that path
  nit one short                         the same 14
  the before / after shortcut with      run_touch fails.  Nothing else does: where two runs touch end to
  <= and < swapped                      end the swap flips the tie on both sides and only exchanges two
                                        equal keys; run_touch puts the touch on a tile edge inside a run,
                                        where one side alone takes the shortcut (the case was added
                                        after this mutant had passed the whole file)
  step_edge_count_kernel without        totals_past_* (w1, w3), edge_diagonals_only (w1, w3) and 9 window_*
  its gap-zero loop                     cases fail (the dirtying steps' totals show through)
  a reciprocal multiply for the         weights, totals_past_*, edge_empty_tile (w1, w3), ties_*, 6 window_*
  two divisions                         cases, world_9 fail
  is_head true at every tile's          ties_*, world_9, run_lengths and 5 window_* cases fail (a group of
  first element                         equal keys across a tile edge is counted twice); the emulated
                                        cases pass, as they must: their lists hold no equal keys
  the slot test > slot - 1 made         slot_kc fails (every rank runs the step again)
  >= slot - 1
slot_kc_plus_1 was left out of the runs of the three merge mutants: a merge
that corrupts the owners' lists differently makes one rank's deferred check
return an error while the others enter the re-run's collectives and wait for
it until the child's time limit.

Measured on an MI355X: the whole file 19 s, the slowest case 1.3 s
(window_pow2; eight rank threads in a child process); on a machine busy with
other work 99 s and 9.5 s (world_9).  merge_stride is built: its batch and
dirtying batches (1.06M contigs, 4.3M + 5.3M + 6.4M records) take about 3 s
on the CPU, the case 1.1 s on the GPU.
"""
import numpy as np
import pytest

import step_tail_reference as st
from karma_amd import _lib, engine
from karma_amd.comm import SoloComm
from karma_amd.distributed import NativeStep
from test_gpu_fake_rccl import run_child

pytestmark = pytest.mark.gpu

SEED = 43


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def dev_records(ctx, rec, flagged):
    if not len(rec):
        return _lib.DevBuf(ctx, (0,), np.int64)
    return _lib.DevBuf.from_numpy(ctx, engine.flag_records(rec) if flagged
                                  else np.ascontiguousarray(rec).view(np.int64).reshape(-1))


def check_edges(e, m):
    assert np.array_equal(e.a, m.a) and np.array_equal(e.b, m.b)
    assert np.array_equal(e.shared, m.shared)
    assert np.array_equal(e.weight.view(np.uint64), m.weight.view(np.uint64))
    assert np.array_equal(e.totals, m.totals)


def run_emulated(ctx, c):
    m = st.graph([c.batch], c.N)  # the model first; the builder has asserted the placement
    blob, offs, kl = engine.synth_contigs(SEED, c.n_loc, 30, 40, 0, first=c.bounds[c.rank])
    store = engine.ContigStore(ctx, blob, offs, kl)
    step = NativeStep(ctx, SoloComm(), -1, c.N, c.bounds, c.rank, c.n_loc)
    steps = [st.records(c.dirt[0], 1), st.records(c.dirt[1], 2), c.rec]
    bufs = [dev_records(ctx, r, c.flagged) for r in steps]
    try:
        for r, d in zip(steps, bufs):
            step.run(store, d.ptr, len(r), count=False, flagged=c.flagged)
        step.sync()
        info = step.info()
        e, deferred = step.newest_edges()
        # three deferred calls (the two tails' dirtying steps, then the case on
        # the first one's tail), nothing synchronous, nothing run again
        assert deferred and info[[4, 5, 6, 7]].tolist() == [0, 3, 0, 0], info.tolist()
        assert int(info[1]) == len(m.a)
        check_edges(e, m)
    finally:
        step.close()
        store.close()
        for d in bufs:
            d.close()


@pytest.mark.parametrize("name", sorted(st.EMU_CASES))
def test_tail_emulated_owners(ctx, name):
    run_emulated(ctx, st.emu_case(name))


def test_tail_edge_stage_second_round(ctx):
    k = _lib.step_tail_tile(ctx)
    assert k.edge_blocks > 0 and k.ET == st.ET
    c = st.build_second_round(k.edge_blocks)
    assert -(-c.U // k.ET) > k.edge_blocks
    run_emulated(ctx, c)


def test_tail_merge_more_tiles_than_blocks(ctx):
    k = _lib.step_tail_tile(ctx)
    assert k.merge_blocks > 0 and k.MT == st.MT
    c = st.build_merge_stride(k.merge_blocks)
    assert sum(-(-x // k.MT) for x in c.runs) > k.merge_blocks
    run_emulated(ctx, c)


@pytest.mark.parametrize("name", sorted(st.RANK_CASES))
def test_tail_merge_from_slots(tmp_path, name):
    c = st.rank_case_named(name)
    m = st.graph(c.batches, c.N)
    st.save_rank_case(c, tmp_path / "case.npz")
    # (the child runs for about a second; ranks that disagree about a re-run wait for each other until this limit)
    run_child("--case", "tail", "--world", str(c.W), "--npz", str(tmp_path / "case.npz"), "--out", str(tmp_path),
              timeout=90)
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(c.W)]
    for r, p in enumerate(parts):
        info = p["info"]
        # the sizing step is synchronous; then three deferred calls.  A slice
        # that outgrows its slot: every rank runs that step again, synchronously.
        assert info[[4, 5, 6, 7]].tolist() == ([2, 3, 1, 0] if c.rerun else [1, 3, 0, 0]), (r, info.tolist())
        assert bool(p["deferred"]) == (not c.rerun), r
        assert int(info[13]) == c.W
        assert int(info[1]) == len(p["a"]), r
        assert np.array_equal(p["tot"], m.totals), r
        assert not len(p["a"]) or (p["a"].min() >= c.bounds[r] and p["a"].max() < c.bounds[r + 1])
    e = engine.EdgeArrays(*[np.concatenate([p[k] for p in parts]) for k in ("a", "b", "s", "w")],
                          np.zeros(0, np.uint64), parts[0]["tot"])
    check_edges(e, m)
