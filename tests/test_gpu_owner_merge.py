"""The exchange owner's merge, split and edge stage against a plain model.

graph.hip's owner path -- merge_bounds_kernel, merge_rank_kernel,
group_count_kernel / group_sum_kernel (compact_pairs), split_kernel,
split_kc_kernel, interleave_kc_kernel / deinterleave_kc_kernel,
diag_totals_kernel, and edges_count_kernel / edges_write_kernel / block_place
fed a merged list -- on inputs built (tests/exchange_reference.py) to land on
the kernels' limits.  Every case goes in as host arrays, as device arrays and
in the interleaved wire format (the last two leave equal keys unsummed up to
64 runs), and every comparison is exact, against the model: the list, its
count, the wire format round trip, split and split_kc at 1..1,023 ranks,
the totals, and the edges (a, b, shared, weight bits, totals over all N) of
the unsummed and of the summed list, in one call, in two halves, and with
the count deferred to the first read.

Which branch each case pins:
  tile_lengths, empty_*, one_run,     runs of 1, TILE - 1, TILE, TILE + 1, 2 TILE, 2 TILE + 1 elements; empty
  one_key, all_empty                  runs first, in the middle and last; no tile at all (no launch)
  ties_2 / 3 / 63 / 64                the same keys in every run: <= before, < after keeps run order; the
                                      group sums over 2..64 elements
  repeat_in_run, all_identical        equal keys inside a run, across its tile edge; one group of 65,600
  bound_L_le / _lt, bound_dup_*       the MG-way bound search on a range of exactly L = 1, MG - 1, MG,
                                      MG + 1, ..., MG^3 + 1 keys with every answer 0..L (single-key runs),
                                      and the in-window search with every answer 0..L
  window_6143 / 6144 / 6145,          a window that fills the LDS stage less one, exactly, and one over
  window_3072_*, window_spill_*       (searched in place); two windows at the limit; a spilled window does
                                      not advance the fill, the next small one is staged
  runs_65 / 129 / 4097                more than 64 runs: two and three levels, a lone run carried by copy,
                                      empty runs inside a group, a group that is all empty
  order_ok_*, UNSORTED                the order check at a tile edge, at a run's end, in the last run, in a
                                      lone run; not across run boundaries, not on equal keys
  totals_last_plus_*, slice*          the count kernel's totals fill (no memset precedes it): contigs before
                                      the first key, gaps of 1, 2 and 1,500, a contig without a diagonal,
                                      1, 2 and 5,000 contigs past the last, an owner's slice of 100,000;
                                      each on a cached totals buffer that the run before left nonzero
  edges_n_*, edges_group_across_*,    the edge stage at n = ET - 1, ET, ET + 1; a group of equal keys over
  edges_empty_block, *_only           elements ET - 1 | ET; a block without an edge between two with; E = 0
  weights                             counts and totals above 2^53 (the conversion rounds), >= 100
                                      divisions that a reciprocal multiply gets wrong, pairs of count 0
Every case asserts its path from the launch counts (merge_launches): an input
that misses its path fails.

all_identical sums 65,600 counts in one thread (twice per edge stage, once per
group sum); the whole case, three input forms, took 0.23 s on an MI355X.
"""
import ctypes

import numpy as np
import pytest

import exchange_reference as xr
from karma_amd import _lib, engine
from test_gpu_pair_buckets import launches

pytestmark = pytest.mark.gpu

READS, EQ = _lib.KARMA_MODE_READS, _lib.KARMA_MODE_EQ
FORMS = ("host", "device", "kc")
MERGE_KERNELS = ("merge_bounds", "merge_rank", "merge_split", "merge_groups", "merge_sum")
RANKS = (1, 2, 255, 256, 257, 1023)   # 1,023: the limit of karma_pairs_split_kc


class Inputs:
    """A case's runs in device memory: separate arrays and the wire format."""

    def __init__(self, ctx, c):
        self.ctx, self.c, self.n = ctx, c, len(c.keys)
        self.keys = _lib.DevBuf.from_numpy(ctx, c.keys)
        self.counts = _lib.DevBuf.from_numpy(ctx, c.counts)
        self.kc = _lib.DevBuf.from_numpy(ctx, np.stack([c.keys.view(np.int64), c.counts], 1).reshape(-1))

    def merge(self, form):
        c = self.c
        if form == "host":
            return engine.Pairs.merge(self.ctx, c.keys, c.counts, runs=c.runs)
        if form == "device":
            return engine.Pairs.merge(self.ctx, self.keys.ptr if self.n else None,
                                      self.counts.ptr if self.n else None, device=True, n=self.n, runs=c.runs)
        return engine.Pairs.merge_runs_kc(self.ctx, self.kc.ptr if self.n else None, c.runs)

    def close(self):
        for b in (self.keys, self.counts, self.kc):
            b.close()


def lazy(form, c):
    return form != "host" and len(c.runs) <= xr.MAX_RUNS


def merge_kernels(n_launch):
    return {k: n_launch.get(k, 0) for k in MERGE_KERNELS}


def run_edges(p, flavour, mode, N, totals_ptr=None, between=None):
    """One edge stage -> (EdgeArrays, None), or (the stage's totals or None, the error's code)."""
    if flavour == "edges":
        try:
            e = p.edges(mode, N, totals_ptr)
        except _lib.KarmaError as err:
            return None, err.code
    else:
        e, tp = p.edges_begin(mode, N)
        if between:
            between(tp)
    try:
        try:
            if flavour != "edges":
                e.end(count=flavour == "end")
            return e.get(), None
        except _lib.KarmaError as err:  # the stage is over; its totals are still there
            t = np.zeros(max(N, 1), np.int64)
            _lib.call("karma_edges_totals", e.h, _lib.ptr(t), 0)
            return t[:N], err.code
    finally:
        e.close()


def check_edges(e, m):
    assert np.array_equal(e.a, m.a) and np.array_equal(e.b, m.b)
    assert np.array_equal(e.shared, m.shared)
    assert np.array_equal(e.weight.view(np.uint64), m.weight.view(np.uint64))
    assert np.array_equal(e.totals, m.totals)


def check_edge_result(got, code, m, what):
    if m.zero_div:
        assert code == _lib.KARMA_ERR_ZERO_DIV, what
        if got is not None:
            assert np.array_equal(got, m.totals), what
    else:
        assert code is None, (what, code)
        check_edges(got, m)


class Dirt:
    """An edge stage of N contigs whose totals are all nonzero, run and closed:
    the context's allocation cache then hands the next stage of N a used buffer."""

    def __init__(self, ctx, N):
        d = np.arange(N, dtype=np.uint64)
        self.N = N
        self.p = engine.Pairs.merge(ctx, xr.key(d, d), np.full(N, 0x5A5A5A5A5A5A, np.int64), runs=[N])

    def __call__(self):
        e = self.p.edges(READS, self.N)
        try:
            assert e.get().totals.all()
        finally:
            e.close()

    def close(self):
        self.p.close()


def check_edge_stage(ctx, p, name, what, dirt, caller_totals):
    c = xr.case(name)
    want = 1 if len(c.keys) else 0
    for flavour in ("edges", "end", "deferred"):
        if dirt:
            dirt()
        n_launch, (got, code) = launches(ctx, lambda: run_edges(p, flavour, READS, c.N))
        assert (n_launch.get("edge_count", 0), n_launch.get("edge_weights", 0)) == (want, want), (what, flavour)
        assert not any(merge_kernels(n_launch).values()), (what, flavour)  # the edge stage sums groups itself
        check_edge_result(got, code, xr.case_edges(name), (what, flavour))
    # KARMA_MODE_EQ with the caller's totals: the diagonal keys are edges too
    got, code = run_edges(p, "edges", EQ, c.N, caller_totals.ptr)
    check_edge_result(got, code, xr.case_edges(name, EQ, True), (what, "eq"))


def bounds_for(c, u, nranks, rng):
    """nranks + 1 owner bounds from 0 to N: on contigs of the list, on absent ones
    next to them and inside gaps, anywhere, and repeated."""
    a = np.unique(xr.ab(u)[0])
    pool = np.r_[a, np.minimum(a + 1, c.N), rng.integers(0, c.N + 1, 64)]
    return np.r_[0, np.sort(rng.choice(pool, nranks - 1)), c.N].astype(np.int64)


def check_form(ctx, inp, name, form, dirt, caller_totals):
    c = inp.c
    u, cnt = xr.case_model(name)
    N, kc_pair = c.N, form == "kc"
    n_launch, p = launches(ctx, lambda: inp.merge(form))
    try:
        assert merge_kernels(n_launch) == xr.merge_launches(c.runs, kc=kc_pair, lazy=lazy(form, c)), (form, n_launch)
        tot = _lib.DevBuf.from_numpy(ctx, np.full(N, -1, np.int64))
        if lazy(form, c):
            # the unsummed list: totals and the edge stage sum its groups themselves
            p.totals_device(tot.ptr, N)
            assert np.array_equal(tot.numpy(), xr.totals(u, cnt, N)), form
            check_edge_stage(ctx, p, name, (form, "unsummed"), dirt, caller_totals)
            n_launch, got = launches(ctx, p.get)  # the first accessor sums the groups (compact_pairs)
            want = 1 if len(c.keys) else 0
            assert merge_kernels(n_launch) == {"merge_bounds": 0, "merge_rank": 0, "merge_split": 0,
                                               "merge_groups": want, "merge_sum": want}, (form, n_launch)
        else:
            got = p.get()
        assert np.array_equal(got[0], u) and np.array_equal(got[1], cnt), form
        n_launch, n = launches(ctx, p.count)
        assert n == len(u) and not any(merge_kernels(n_launch).values()), form
        # the wire format, alone and with the split
        kc = _lib.DevBuf.from_numpy(ctx, np.full(2 * len(u), -1, np.int64))
        wire = np.stack([u.view(np.int64), cnt], 1).reshape(-1)
        p.get_kc(kc.ptr if len(u) else None)
        assert np.array_equal(kc.numpy(), wire), form
        rng = np.random.default_rng(len(name))
        for nranks in RANKS:
            b = bounds_for(c, u, nranks, rng)
            assert np.array_equal(p.split(b), xr.split(u, b)), (form, nranks)
            kc.copy_from(np.full(2 * len(u), -1, np.int64))
            n_launch, starts = launches(ctx, lambda: p.split_kc(b, kc.ptr))
            assert n_launch.get("pairs_split_kc", 0) == 1
            assert np.array_equal(starts, xr.split(u, b)), (form, nranks)
            assert np.array_equal(kc.numpy(), wire), (form, nranks)
        kc.close()
        tot.copy_from(np.full(N, -1, np.int64))
        p.totals_device(tot.ptr, N)
        assert np.array_equal(tot.numpy(), xr.totals(u, cnt, N)), form
        tot.close()
        check_edge_stage(ctx, p, name, (form, "summed"), dirt, caller_totals)
    finally:
        p.close()


@pytest.mark.parametrize("name", sorted(xr.CASES))
def test_owner_merge_case(name):
    c = xr.case(name)
    ctx = _lib.default_context()
    inp = Inputs(ctx, c)
    dirt = Dirt(ctx, c.N) if name in xr.TOTALS_FILL else None
    caller_totals = _lib.DevBuf.from_numpy(ctx, 1000 + 3 * np.arange(c.N, dtype=np.int64))
    try:
        for form in FORMS:
            check_form(ctx, inp, name, form, dirt, caller_totals)
    finally:
        caller_totals.close()
        inp.close()
        if dirt:
            dirt.close()


@pytest.mark.parametrize("name", sorted(xr.UNSORTED))
def test_descent_inside_a_run_is_reported(name):
    """KARMA_ERR_UNSORTED: from the call for host arrays and past 64 runs; from
    the first accessor, the edge stage and the deferred read for the forms that
    return without a synchronisation.  The context works afterwards."""
    c = xr.case(name)
    ctx = _lib.default_context()
    inp = Inputs(ctx, c)
    try:
        for form in FORMS:
            if not lazy(form, c):
                with pytest.raises(_lib.KarmaError) as ei:
                    inp.merge(form)
                assert ei.value.code == _lib.KARMA_ERR_UNSORTED, form
                continue
            for use in ("get", "count", "edges", "end", "deferred"):
                p = inp.merge(form)
                try:
                    if use in ("get", "count"):
                        with pytest.raises(_lib.KarmaError) as ei:
                            getattr(p, use)()
                        code = ei.value.code
                    else:
                        _, code = run_edges(p, use, READS, c.N)
                    assert code == _lib.KARMA_ERR_UNSORTED, (form, use)
                finally:
                    p.close()
    finally:
        inp.close()
    good = xr.case("one_key")
    p = engine.Pairs.merge(ctx, good.keys, good.counts, runs=good.runs)
    assert np.array_equal(p.get()[0], good.keys)
    p.close()


def owner_lists(ctx, inp):
    """The owner's merged list, unsummed and summed."""
    lazy_p = inp.merge("kc")
    summed = inp.merge("kc")
    assert summed.count() < inp.n
    return {"unsummed": lazy_p, "summed": summed}


@pytest.mark.parametrize("flavour", ["end", "deferred"])
def test_owner_flow_end_reads_the_totals_the_caller_gathered(flavour):
    """edges_begin -> the caller overwrites slices of the returned device totals
    (the all-gather of the other owners' readset sizes) -> end: weights and
    totals are those of the overwritten array.  The list's b reach into other
    owners' slices, whose totals are 0 until then; one of the owner's own totals
    is overwritten too."""
    name = "slice_zero_div"
    c = xr.case(name)
    ctx = _lib.default_context()
    m0 = xr.case_edges(name)
    assert m0.zero_div
    rng = np.random.default_rng(5)
    tot = m0.totals.copy()
    tot[41_000:] = rng.integers(1, 1 << 40, c.N - 41_000)
    tot[:40_000] = rng.integers(1, 1 << 40, 40_000)
    own = int(m0.a[10])
    tot[own] = 12_345
    m = xr.edges(c.keys, c.counts, c.N, READS, tot)
    assert not m.zero_div and not np.array_equal(m.weight, m0.weight)

    def gather(tp):
        for lo, hi in ((0, 40_000), (41_000, c.N), (own, own + 1)):
            part = np.ascontiguousarray(tot[lo:hi])
            _lib.call("karma_memcpy", ctx.h, ctypes.c_void_p(tp + 8 * lo), _lib.ptr(part), part.nbytes, 0)

    inp = Inputs(ctx, c)
    dirt = Dirt(ctx, c.N)
    lists = owner_lists(ctx, inp)
    try:
        for what, p in lists.items():
            dirt()
            got, code = run_edges(p, flavour, READS, c.N, between=gather)
            assert code is None, what
            check_edges(got, m)
    finally:
        for p in lists.values():
            p.close()
        dirt.close()
        inp.close()


@pytest.mark.parametrize("flavour", ["end", "deferred"])
def test_owner_flow_zero_total_written_by_the_caller(flavour):
    """One used total set to 0 between edges_begin and end: KARMA_ERR_ZERO_DIV
    from end(), or from the first read after end(count=False); the stage's
    totals show the 0, and the context works afterwards."""
    name = "slice"
    c = xr.case(name)
    ctx = _lib.default_context()
    m0 = xr.case_edges(name)
    assert not m0.zero_div
    used = int(m0.b[len(m0.b) // 2])
    tot = m0.totals.copy()
    tot[used] = 0

    def zero(tp):
        z = np.zeros(1, np.int64)
        _lib.call("karma_memcpy", ctx.h, ctypes.c_void_p(tp + 8 * used), _lib.ptr(z), 8, 0)

    inp = Inputs(ctx, c)
    lists = owner_lists(ctx, inp)
    try:
        for what, p in lists.items():
            got, code = run_edges(p, flavour, READS, c.N, between=zero)
            assert code == _lib.KARMA_ERR_ZERO_DIV, what
            assert np.array_equal(got, tot), what
            got, code = run_edges(p, flavour, READS, c.N)  # the same list and context, untouched totals
            assert code is None, what
            check_edges(got, m0)
    finally:
        for p in lists.values():
            p.close()
        inp.close()
