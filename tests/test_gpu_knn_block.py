"""The blockwise neighbour lists on the GPU (karma_knn_block, karma_knn_merge,
karma_knn_finish; engine.KnnState, engine.knn_blocked, distributed.knn_sharded)
against the numpy model (tests/knn_block_reference.py): every comparison is on
the bits of idx, of the keys and of dist.  Sizes come from the kernel's tile as
karma_knn_tile reports it (q query rows, c candidate rows, p staged columns).

Groups: A block order and ties, B one update against arbitrary carried state,
C the candidate split, D merge and finish, E index range and errors, F pointer
locations and strides, G equivalence with karma_knn_rows, H ranks."""
import ctypes

import numpy as np
import pytest

import knn_block_reference as blk
import knn_reference as ref
from karma_amd import _lib, engine
from karma_amd.comm import HostComm, SoloComm
from karma_amd.distributed import ShardedBuild, knn_sharded
from karma_amd.hostgroup import run_ranks

pytestmark = pytest.mark.gpu

U64 = np.uint64
MAX_INDEX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def _tile():
    return _lib.knn_tile()


def _resolve(name):
    q, c, p, _ = _tile()
    named = {"q-1": q - 1, "q": q, "q+1": q + 1, "c-1": c - 1, "c": c, "c+1": c + 1, "2c+3": 2 * c + 3,
             "p-1": p - 1, "p": p, "p+1": p + 1}
    return named[name] if name in named else int(name)


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == wi.shape == gd.shape
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(U64), wd.view(U64))


def _same_state(got, want):
    gk, gi = got
    wk, wi = want
    assert gk.dtype == U64 and gi.dtype == np.int32 and gk.shape == wk.shape == gi.shape
    assert np.array_equal(gi, wi)
    assert np.array_equal(gk, wk)


def P(a):
    """A host array's or a device buffer's address (None stays None)."""
    if a is None or isinstance(a, ctypes.c_void_p):
        return a
    return ctypes.c_void_p(a.ptr) if isinstance(a, _lib.DevBuf) else _lib.ptr(a)


def D(a):
    return 1 if isinstance(a, _lib.DevBuf) else 0


def raw_block(ctx, q, c, base, k, keys, idx, first, split=1, over=None):
    """karma_knn_block as it is declared; `over` replaces arguments by name."""
    a = dict(q=P(q), nq=q.shape[0], ldq=q.shape[1], qdev=D(q), c=P(c), nc=c.shape[0], ldc=c.shape[1], cdev=D(c),
             m=q.shape[1], base=base, k=k, keys=P(keys), idx=P(idx), sdev=D(keys), first=first, split=split)
    a.update(over or {})
    _lib.call("karma_knn_block", ctx.h, a["q"], a["nq"], a["ldq"], a["qdev"], a["c"], a["nc"], a["ldc"], a["cdev"],
              a["m"], a["base"], a["k"], a["keys"], a["idx"], a["sdev"], a["first"], a["split"])


def launches(ctx, fn):
    """fn() with every launch counted: ({kernel name: launches}, fn's result)."""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        out = fn()
        return {k: v[1] for k, v in ctx.timing_read(256).items()}, out
    finally:
        ctx.timing(False)


def garbage(nq, k):
    """A state that must not be read (first = 1)."""
    return np.full((nq, k), 0x0123456789ABCDEF, U64), np.full((nq, k), -77, np.int32)


# ---- A. block order and ties ---------------------------------------------------

def _dup_matrix():
    _, c, _, _ = _tile()
    n, m, k = 2 * c + 40, 5, 8
    x = np.random.default_rng(9).random((n, m))
    at = [4, 11, 50, c - 2, c - 1, c, c + 1, c + 9, c + 77, 2 * c - 1, 2 * c, 2 * c + 1, 2 * c + 7, 2 * c + 30,
          2 * c + 38, 2 * c + 39]
    assert len(at) == 2 * k and {i // c for i in at} == {0, 1, 2}
    x[at] = x[at[0]]
    return x, k


@pytest.fixture(scope="module")
def tie_cases():
    out = {}
    for name, (x, k) in (("lattice", (ref.tie_lattice(), 8)), ("duplicates", _dup_matrix())):
        want = ref.knn(x, k)
        for a in (x,) + want:
            a.setflags(write=False)
        out[name] = (x, k, want)
    return out


def _pieces(n, piece):
    return list(range(0, n, piece)) + [n]


@pytest.mark.parametrize("piece_at", ["1", "c-1", "c", "c+1"])
@pytest.mark.parametrize("name", ["lattice", "duplicates"])
def test_block_order_and_ties(ctx, tie_cases, name, piece_at):
    x, k, want = tie_cases[name]
    n, m = x.shape
    _, c, _, _ = _tile()
    assert x.shape == (257, 9) and k == 8 if name == "lattice" else n > 2 * c
    piece = _resolve(piece_at)
    cuts = _pieces(n, piece)
    nb = len(cuts) - 1
    assert nb >= 2 and (cuts[1] - cuts[0] == piece)
    dev = _lib.DevBuf.from_numpy(ctx, x)
    try:
        orders = {"ascending": list(range(nb)), "descending": list(range(nb))[::-1],
                  "shuffled": np.random.default_rng(nb).permutation(nb).tolist()}
        for what, order in orders.items():
            st = engine.KnnState(ctx, n, k)
            try:
                for b in order:
                    lo, hi = cuts[b], cuts[b + 1]
                    st.update(dev, dev.view(lo * m, (hi - lo) * m, shape=(hi - lo, m)), lo, cand_split=1)
                got = st.finish()
            finally:
                st.close()
            assert np.array_equal(got[0], want[0]), (what, piece)
            _same(got, want)
    finally:
        dev.close()


# ---- B. one update against arbitrary carried state -------------------------------

def carried_state(rng, bits, base, k, mode):
    """A synthetic sorted state for queries whose block d2 bits are `bits`
    (nq x nc), with no index inside [base, base + nc).  mode: full | partial |
    empty | inf.  Half of the entries take a key of the block (an equal d2),
    with indices both below and above the block's."""
    nq, nc = bits.shape
    keys, idx = blk.empty(nq, k)
    if mode == "empty":
        return keys, idx
    below = np.arange(0, base)
    above = np.arange(base + nc, base + nc + 4 * k + 8)
    pool = np.concatenate([below[-(2 * k + 4):], above]) if len(below) else above
    scale = float(bits.view(np.float64).max()) if nc else 1.0
    scale = scale if np.isfinite(scale) and scale > 0 else 1.0
    for r in range(nq):
        fill = k if mode in ("full", "inf") else int(rng.integers(0, k))
        ii = rng.choice(pool, fill, replace=False)
        kk = (rng.random(fill) * scale).view(U64)
        if nc:
            eq = rng.random(fill) < 0.5
            kk = np.where(eq, bits[r, rng.integers(0, nc, fill)], kk)
        if mode == "inf" and fill:
            kk[rng.random(fill) < 0.4] = np.float64(np.inf).view(U64)
        o = np.lexsort((ii, kk))
        keys[r, :fill], idx[r, :fill] = kk[o], ii[o]
    return keys, idx


B_CASES = [
    # nq, nc, m, k, mode
    ("1", "1", "0", 1, "first"),
    ("1", "2c+3", "1", 2, "full"),
    ("q-1", "q", "p-1", 15, "full"),
    ("q", "q+1", "p", 15, "partial"),
    ("q+1", "q-1", "p+1", 64, "full"),
    ("2c+3", "1", "64", 15, "inf"),
    ("q", "0", "p", 15, "partial"),
    ("q+1", "0", "p+1", 2, "first"),
    ("q-1", "1", "1", 2, "empty"),
    ("q", "14", "p+1", 15, "partial"),   # nc = k - 1
    ("q+1", "63", "64", 64, "empty"),    # nc = k - 1
    ("2c+3", "2c+3", "64", 64, "inf"),
    ("2c+3", "2c+3", "0", 15, "full"),
    ("1", "q", "64", 1, "full"),
    ("2c+3", "q+1", "p", 1, "first"),
]


@pytest.mark.parametrize("nq_at,nc_at,m_at,k,mode", B_CASES)
def test_one_update_against_carried_state(ctx, nq_at, nc_at, m_at, k, mode):
    q_, c_, p_, k_max = _tile()
    nq, nc, m = _resolve(nq_at), _resolve(nc_at), _resolve(m_at)
    assert k <= k_max
    rng = np.random.default_rng(7919 * nq + 31 * nc + m + k)
    big = mode == "inf"
    q = rng.random((nq, m))
    c = rng.random((nc, m))
    if big and m:
        c[rng.random(nc) < 0.3, 0] = 1e160  # finite, its square is not: +inf d2 inside the block too
    base = 5000
    bits = np.ascontiguousarray(blk.d2_block(q, c)).view(U64).reshape(nq, nc)
    if mode == "first":
        keys, idx = garbage(nq, k)
        want = blk.update(None, None, q, c, base, k)
    else:
        keys, idx = carried_state(rng, bits, base, k, mode)
        want = blk.update(keys, idx, q, c, base, k)
        if mode == "full" and nc and m and nq > 16:
            # the case the index decides: a carried key equal to a block d2, with indices on both sides
            eq = (keys[:, :, None] == bits[:, None, :]).any(axis=2)
            assert (eq & (idx < base)).any() and (eq & (idx >= base + nc)).any()
    raw_block(ctx, q, c, base, k, keys, idx, 1 if mode == "first" else 0)
    _same_state((keys, idx), want)
    assert (np.lexsort((idx[0], keys[0])) == np.arange(k)).all()  # sorted by (key, index), empties last


# ---- C. the candidate split ------------------------------------------------------

@pytest.mark.parametrize("tiles", [3, 9])
def test_candidate_split(ctx, tiles):
    q_, c_, p_, _ = _tile()
    nq, nc, m, k = q_ + 5, tiles * c_ - 7, p_ + 1, 15
    assert (nc + c_ - 1) // c_ == tiles and nc % c_ != 0  # the last tile is partial
    rng = np.random.default_rng(100 + tiles)
    q, c = rng.random((nq, m)), rng.random((nc, m))
    base = 3000
    bits = np.ascontiguousarray(blk.d2_block(q, c)).view(U64).reshape(nq, nc)
    carried = carried_state(rng, bits, base, k, "full")
    want_first = blk.update(None, None, q, c, base, k)
    want_carried = blk.update(*carried, q, c, base, k)
    for S in (1, 2, 3, 7, 1000):
        used = _lib.knn_block_split(ctx, nq, nc, S)
        assert used == min(S, tiles, 32)
        for first, want in ((1, want_first), (0, want_carried)):
            keys, idx = garbage(nq, k) if first else (carried[0].copy(), carried[1].copy())
            n_launch, _ = launches(ctx, lambda: raw_block(ctx, q, c, base, k, keys, idx, first, split=S))
            _same_state((keys, idx), want)  # identical to S = 1 and to the model
            assert n_launch.get("profile_knn_block", 0) == 1
            assert n_launch.get("profile_knn_merge", 0) == (1 if used > 1 else 0), (S, n_launch)


def test_candidate_split_auto(ctx):
    nq, nc, m, k = 300, 20_000, 64, 15
    assert _lib.knn_block_split(ctx, nq, nc, 0) > 1  # a small query shard is split to fill the chip
    rng = np.random.default_rng(300)
    q, c = rng.random((nq, m)), rng.random((nc, m))
    want = blk.update(None, None, q, c, 0, k)
    keys, idx = garbage(nq, k)
    n_launch, _ = launches(ctx, lambda: raw_block(ctx, q, c, 0, k, keys, idx, 1, split=0))
    _same_state((keys, idx), want)
    assert n_launch.get("profile_knn_block", 0) == 1 and n_launch.get("profile_knn_merge", 0) == 1


# ---- D. merge and finish ---------------------------------------------------------

def test_merge_two_lists_with_ties_and_empties(ctx):
    q_, _, _, _ = _tile()
    rng = np.random.default_rng(41)
    for nq, k in ((1, 1), (q_ + 3, 15), (7, 64)):
        a, b = blk.empty(nq, k), blk.empty(nq, k)
        for r in range(nq):
            fa, fb = (int(rng.integers(0, k + 1)) for _ in range(2))
            if r == 0:
                fa, fb = k, k
            if r == 1:
                fa, fb = 0, 0
            ii = rng.permutation(4 * k)[:fa + fb] + 10
            kk = rng.integers(0, 6, fa + fb).astype(np.float64).view(U64)  # few distinct keys: ties across the lists
            kk[rng.random(fa + fb) < 0.2] = np.float64(np.inf).view(U64)
            for (dk, di), sl in ((a, slice(0, fa)), (b, slice(fa, fa + fb))):
                o = np.lexsort((ii[sl], kk[sl]))
                dk[r, :len(o)], di[r, :len(o)] = kk[sl][o], ii[sl][o]
        want = blk.merge(*a, *b)
        # host lists
        keys, idx = a[0].copy(), a[1].copy()
        _lib.call("karma_knn_merge", ctx.h, P(keys), P(idx), P(b[0]), P(b[1]), nq, k, 0)
        _same_state((keys, idx), want)
        # device lists; the second list is left as it was
        dk, di, ek, ei = (_lib.DevBuf.from_numpy(ctx, v) for v in (a[0], a[1], b[0], b[1]))
        try:
            n_launch, _ = launches(ctx, lambda: _lib.call("karma_knn_merge", ctx.h, P(dk), P(di), P(ek), P(ei), nq, k, 1))
            assert n_launch == {"profile_knn_merge": 1}
            _same_state((dk.numpy(), di.numpy()), want)
            _same_state((ek.numpy(), ei.numpy()), b)
        finally:
            for v in (dk, di, ek, ei):
                v.close()


def test_state_merge_is_the_update_with_both(ctx):
    _, c_, _, _ = _tile()
    n, m, k = c_ + 30, 9, 15
    x = ref.profile_like(np.random.default_rng(43), n, m)
    want = ref.knn(x, k)
    a, b, e = (engine.KnnState(ctx, n, k) for _ in range(3))
    try:
        a.update(x, x[:50], 0)
        b.update(x, x[50:], 50)
        e.merge(a)  # into an untouched state: a copy
        e.merge(b)
        a.merge(b)
        assert a.rows_seen == e.rows_seen == n
        _same(a.finish(), want)
        _same(e.finish(), want)
    finally:
        for s in (a, b, e):
            s.close()


def test_finish_bits(ctx):
    k = 8
    d2 = np.array([0.0, 5e-324, 2.5e-310, np.finfo(np.float64).tiny, 2.0, 1e300, 1.7976931348623157e308, np.inf])
    keys = np.stack([d2.view(U64), d2.view(U64), blk.empty(1, k)[0][0]])
    idx = np.stack([np.arange(k, dtype=np.int32), (np.arange(k) + (MAX_INDEX - k)).astype(np.int32),
                    blk.empty(1, k)[1][0]])
    keys[1, 5:], idx[1, 5:] = blk.NO_KEY, blk.NO_IDX  # partly empty
    want = blk.finish(keys, idx)
    assert want[0][2].tolist() == [-1] * k and np.isposinf(want[1][2]).all() and np.isposinf(want[1][0, 7])
    assert want[0][0, 7] == 7 and 0 < want[1][0, 1] < 1e-150  # +inf d2 is no empty slot; sqrt of a subnormal
    oi, od = np.full((3, k), -9, np.int32), np.full((3, k), -9.0)
    _lib.call("karma_knn_finish", ctx.h, P(keys), P(idx), 3, k, 0, P(oi), P(od), 0)
    _same((oi, od), want)


# ---- E. index range and errors ---------------------------------------------------

def test_largest_indices(ctx):
    _, c_, _, _ = _tile()
    nq, nc, m, k = 5, c_ + 9, 3, 15
    rng = np.random.default_rng(47)
    q, c = rng.random((nq, m)), rng.random((nc, m))
    base = MAX_INDEX - nc
    want = blk.update(None, None, q, c, base, k)
    assert base + nc - 1 == 2 ** 31 - 2
    c[-1] = q[0]  # the last index is row 0's nearest
    want = blk.update(None, None, q, c, base, k)
    assert want[1][0, 0] == 2 ** 31 - 2
    for S in (1, 2):
        keys, idx = garbage(nq, k)
        raw_block(ctx, q, c, base, k, keys, idx, 1, split=S)
        _same_state((keys, idx), want)
    # a carried entry at the largest index, folded with a block below it
    keys, idx = want[0].copy(), want[1].copy()
    raw_block(ctx, q, c[:7], 10, k, keys, idx, 0)
    _same_state((keys, idx), blk.update(*want, q, c[:7], 10, k))


def test_argument_errors_and_messages(ctx):
    nq, nc, m, k = 6, 9, 4, 3
    rng = np.random.default_rng(53)
    q, c = rng.random((nq, m)), rng.random((nc, m))
    keys, idx = garbage(nq, k)
    cases = [(dict(base=MAX_INDEX - nc + 1), "cand_base + nc <= 2^31 - 1"), (dict(base=-1), "0 <= cand_base"),
             (dict(k=0), "1 <= k <= 64"), (dict(k=65), "1 <= k <= 64"),
             (dict(ldq=m - 1), "ldq and ldc must be at least m"), (dict(ldc=m - 1), "ldq and ldc must be at least m"),
             (dict(q=None), "null pointer"), (dict(c=None), "null pointer"), (dict(keys=None), "null pointer"),
             (dict(idx=None), "null pointer"),
             (dict(q=ctypes.c_void_p(q.ctypes.data + 4)), "8-byte aligned"),
             (dict(keys=ctypes.c_void_p(keys.ctypes.data + 4)), "8-byte aligned"),
             (dict(idx=ctypes.c_void_p(idx.ctypes.data + 2)), "4-byte aligned"),
             (dict(nq=-1), "must not be negative"), (dict(nc=-1), "must not be negative"),
             (dict(split=-1), "cand_split must not be negative"),
             (dict(nc=1 << 20, ldc=1 << 40), "byte size overflows")]

    def call(first, **kw):
        raw_block(ctx, q, c, 0, k, keys, idx, first, over=kw)

    for kw, text in cases:
        for first in (0, 1):
            with pytest.raises(_lib.KarmaError) as e:
                call(first, **kw)
            assert e.value.code == _lib.KARMA_ERR_ARG and text in str(e.value), (kw, str(e.value))
            assert "karma_knn_block" in str(e.value)
    g = garbage(nq, k)
    assert np.array_equal(keys, g[0]) and np.array_equal(idx, g[1])  # the state is untouched
    out_i, out_d = np.full((nq, k), -9, np.int32), np.full((nq, k), -9.0)
    for fn, args, text in (
            ("karma_knn_merge", (P(keys), P(idx), None, P(idx), nq, k, 0), "null pointer"),
            ("karma_knn_merge", (P(keys), P(idx), P(keys), P(idx), nq, 65, 0), "1 <= k <= 64"),
            ("karma_knn_merge", (ctypes.c_void_p(keys.ctypes.data + 4), P(idx), P(keys), P(idx), nq, k, 0), "aligned"),
            ("karma_knn_finish", (P(keys), P(idx), nq, 0, 0, P(out_i), P(out_d), 0), "1 <= k <= 64"),
            ("karma_knn_finish", (P(keys), P(idx), nq, k, 0, None, P(out_d), 0), "null pointer"),
            ("karma_knn_finish", (P(keys), P(idx), -1, k, 0, P(out_i), P(out_d), 0), "must not be negative")):
        with pytest.raises(_lib.KarmaError) as e:
            _lib.call(fn, ctx.h, *args)
        assert e.value.code == _lib.KARMA_ERR_ARG and text in str(e.value) and fn in str(e.value)
    assert np.array_equal(keys, g[0]) and np.array_equal(idx, g[1]) and (out_i == -9).all() and (out_d == -9.0).all()
    # nothing to do is no error: no query rows (pointers and k are not looked at), no candidates after the first call
    call(0, nq=0, q=None, keys=None, idx=None, k=0)
    call(0, nc=0, c=None)
    assert np.array_equal(keys, g[0]) and np.array_equal(idx, g[1])
    call(1, nc=0, c=None)  # with first: all-empty lists
    _same_state((keys, idx), blk.empty(nq, k))
    call(0)
    _same_state((keys, idx), blk.update(None, None, q, c, 0, k))


# ---- F. pointers and strides -------------------------------------------------------

def test_host_and_device_pointers_agree(ctx):
    q_, c_, _, _ = _tile()
    nq, nc, m, k = q_ + 3, c_ + 5, 33, 15
    rng = np.random.default_rng(59)
    q, c = ref.profile_like(rng, nq, m), ref.profile_like(rng, nc, m)
    base = 900
    bits = np.ascontiguousarray(blk.d2_block(q, c)).view(U64).reshape(nq, nc)
    carried = carried_state(rng, bits, base, k, "partial")
    want = blk.update(*carried, q, c, base, k)
    want_out = blk.finish(*want)
    qd, cd = _lib.DevBuf.from_numpy(ctx, q), _lib.DevBuf.from_numpy(ctx, c)
    try:
        for qs in (q, qd):
            for cs in (c, cd):
                for state_dev in (False, True):
                    keys, idx = carried[0].copy(), carried[1].copy()
                    if state_dev:
                        keys, idx = _lib.DevBuf.from_numpy(ctx, keys), _lib.DevBuf.from_numpy(ctx, idx)
                    raw_block(ctx, qs, cs, base, k, keys, idx, 0, split=2 if qs is q else 1)
                    got = (keys.numpy(), idx.numpy()) if state_dev else (keys, idx)
                    _same_state(got, want)
                    for out_dev in (False, True):
                        oi, od = np.empty((nq, k), np.int32), np.empty((nq, k), np.float64)
                        if out_dev:
                            oi, od = _lib.DevBuf(ctx, (nq, k), np.int32), _lib.DevBuf(ctx, (nq, k), np.float64)
                        _lib.call("karma_knn_finish", ctx.h, P(keys), P(idx), nq, k, D(keys), P(oi), P(od), D(oi))
                        _same((oi.numpy(), od.numpy()) if out_dev else (oi, od), want_out)
                        if out_dev:
                            oi.close()
                            od.close()
                    if state_dev:
                        keys.close()
                        idx.close()
    finally:
        qd.close()
        cd.close()


def test_row_stride_padding_is_never_read(ctx):
    q_, c_, p_, _ = _tile()
    nq, nc, m, k = q_ + 5, c_ + 7, p_ + 1, 15
    rng = np.random.default_rng(61)
    wide_q, wide_c = np.full((nq, m + 2), np.nan), np.full((nc, m + 3), np.nan)
    wide_q[:, :m], wide_c[:, :m] = rng.random((nq, m)), rng.random((nc, m))
    want = blk.update(None, None, wide_q[:, :m], wide_c[:, :m], 11, k)
    assert np.isfinite(blk.finish(*want)[1]).all()
    # through the engine: a view keeps its row stride
    assert engine._knn_source(wide_c[:, :m])[4] == m + 3
    st = engine.KnnState(ctx, nq, k)
    try:
        st.update(wide_q[:, :m], wide_c[:, :m], 11)
        _same(st.finish(), blk.finish(*want))
    finally:
        st.close()
    # the padded matrices on the device
    qd, cd = _lib.DevBuf.from_numpy(ctx, wide_q), _lib.DevBuf.from_numpy(ctx, wide_c)
    try:
        keys, idx = garbage(nq, k)
        raw_block(ctx, qd, cd, 11, k, keys, idx, 1, over=dict(m=m))
        _same_state((keys, idx), want)
    finally:
        qd.close()
        cd.close()


# ---- G. equivalence with the shipped entry -----------------------------------------

@pytest.mark.parametrize("m", [64, 1088])
def test_one_block_is_knn_rows(ctx, m):
    _, c_, _, _ = _tile()
    n, k = 2 * c_ + 3, 15
    x = ref.profile_like(np.random.default_rng(67 + m), n, m)
    want = engine.knn_rows(x, k, ctx=ctx)
    st = engine.KnnState(ctx, n, k)
    try:
        st.update(x, x, 0, cand_split=1)
        _same(st.finish(), want)
        di, dd = st.finish(out_device=True)
        _same((di.numpy(), dd.numpy()), want)
        di.close()
        dd.close()
    finally:
        st.close()


def test_knn_blocked_is_knn_rows(ctx):
    q_, _, p_, _ = _tile()
    n, m, k = q_ + 3, p_ + 1, 15
    x = ref.profile_like(np.random.default_rng(71), n, m)
    want = engine.knn_rows(x, k, ctx=ctx)
    _same(want, ref.knn(x, k))
    assert n % 50 != 0
    for block_rows in (1, q_, n, 50):
        _same(engine.knn_blocked(x, k, block_rows, ctx=ctx), want)


# ---- H. ranks ----------------------------------------------------------------------

RANK_BOUNDS = {1: [0, 700], 2: [0, 7, 700], 3: [0, 0, 9, 700], 8: [0, 100, 100, 107, 300, 301, 500, 690, 700]}


@pytest.fixture(scope="module")
def ring_case():
    x = ref.profile_like(np.random.default_rng(73), 700, 64)
    want = ref.knn(x, 15)
    for a in (x,) + want:
        a.setflags(write=False)
    return x, want


def _ring_rank(group, rank, x, bounds, k):
    ctx = _lib.Context(0)
    try:
        comm = HostComm(group) if group.world > 1 else SoloComm()
        local = _lib.DevBuf.from_numpy(ctx, x[bounds[rank]:bounds[rank + 1]])
        assert local.shape == (bounds[rank + 1] - bounds[rank], x.shape[1])
        try:
            return knn_sharded(comm, ctx, local, bounds, k)
        finally:
            local.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_ranks_ring(ring_case, world):
    x, want = ring_case
    bounds, k = RANK_BOUNDS[world], 15
    sizes = np.diff(bounds)
    assert len(bounds) == world + 1 and bounds[-1] == len(x)
    if world > 2:
        assert (sizes == 0).any() and ((sizes > 0) & (sizes < k)).any() and len(set(sizes.tolist())) > 2
    elif world == 2:
        assert ((sizes > 0) & (sizes < k)).any()
    parts = run_ranks(world, _ring_rank, x, bounds, k)
    assert [len(p[0]) for p in parts] == sizes.tolist()
    _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want)


def _build_rank(group, rank, world, seed, n_glob, f_glob, k):
    ctx = _lib.Context(0)
    try:
        c_lo, c_hi = n_glob * rank // world + (3 if 0 < rank < world else 0), \
            n_glob * (rank + 1) // world + (3 if rank + 1 < world else 0)
        f_lo, f_hi = f_glob * rank // world, f_glob * (rank + 1) // world
        blob, offs, key_len = engine.synth_contigs(seed, c_hi - c_lo, 30, 900, 200, first=c_lo)
        rec = engine.synth_records(seed, n_glob, f_lo, f_hi, False)
        build = ShardedBuild(ctx, HostComm(group), engine.kmode_of("5p6"), n_glob, c_lo, c_hi - c_lo)
        store = engine.ContigStore(ctx, blob, offs, key_len)
        rec_dev = _lib.DevBuf.from_numpy(ctx, rec.view(np.int64).reshape(-1))
        try:
            with pytest.raises(ValueError, match="no kept step"):
                build.knn(k)
            with pytest.raises(ValueError, match="1 <= k <= min"):
                build.knn(65)
            res = build.run(store, rec_dev.ptr, len(rec), keep=True)
            idx, dist = build.knn(k)
            return res["profile"].numpy(), idx, dist, build.bounds.tolist()
        finally:
            build.close()
            store.close()
            rec_dev.close()
    finally:
        ctx.close()


def test_sharded_build_knn():
    world, n_glob, k = 2, 700, 15
    parts = run_ranks(world, _build_rank, world, 41, n_glob, 4000, k)
    assert parts[0][3] == parts[1][3] == [0, 353, 700]
    host = np.concatenate([p[0] for p in parts])
    assert host.shape[0] == n_glob and host.shape[1] > 1000
    half = n_glob // 2
    a, b = ref.knn(host, k, 0, half), ref.knn(host, k, half, n_glob)
    _same((np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])),
          (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])))
