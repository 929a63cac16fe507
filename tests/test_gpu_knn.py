"""karma_knn_rows on the GPU against the numpy model (tests/knn_reference.py):
every comparison is on the bits of idx and dist.  Cases are placed on the
kernel's tile edges as karma_knn_tile reports them, and each one first asserts
(from the tile or from the model) that it sits where it claims."""
import ctypes
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest

import knn_reference as ref
from karma_amd import _lib, engine
from karma_amd import kmer as kmer_mod
from karma_amd.kmer import KmerClustering

pytestmark = pytest.mark.gpu

U64 = np.uint64


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def _tile():
    return _lib.knn_tile()


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == wi.shape == gd.shape
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(U64), wd.view(U64))


def _check_ks(x, ks, ctx, row_lo=0, row_hi=None):
    d2 = ref.d2_rows(x, row_lo, row_hi)
    order = ref.order_rows(d2)
    for k in ks:
        _same(engine.knn_rows(x, k, row_lo, row_hi, ctx=ctx), ref.knn_from_d2(d2, order, k))


# ---- 1. tile edges -----------------------------------------------------------

N_AT = ["1", "2", "q-1", "q", "q+1", "c-1", "c", "c+1", "2c+3"]
M_AT = ["1", "p-1", "p", "p+1", "64", "1088"]


def _resolve(name):
    q, c, p, _ = _tile()
    named = {"q-1": q - 1, "q": q, "q+1": q + 1, "c-1": c - 1, "c": c, "c+1": c + 1, "2c+3": 2 * c + 3,
             "p-1": p - 1, "p": p, "p+1": p + 1}
    return named[name] if name in named else int(name)


@pytest.mark.parametrize("m_at", M_AT)
@pytest.mark.parametrize("n_at", N_AT)
def test_tile_edges(ctx, n_at, m_at):
    q, c, p, k_max = _tile()
    n, m = _resolve(n_at), _resolve(m_at)
    # the case sits where its name says, by the library's own geometry
    where = {"1": n == 1, "2": n == 2, "q-1": n % q == q - 1 and n < q, "q": n == q, "q+1": n % q == 1 and n // q == 1,
             "c-1": n % c == c - 1 and n < c, "c": n == c, "c+1": n % c == 1 and n // c == 1,
             "2c+3": n // c == 2 and n % c == 3}
    assert where[n_at]
    assert {"1": m == 1, "p-1": m % p == p - 1 and m < p, "p": m == p, "p+1": m % p == 1 and m // p == 1,
            "64": m == 64, "1088": m == 1088}[m_at]
    if m_at == "1088":
        assert m % p == 0 and m // p > 2  # many whole panels
    ks = sorted({k for k in (1, 2, 15, min(n, k_max)) if k <= n})
    rng = np.random.default_rng(1000 * n + m)
    _check_ks(rng.random((n, m)), ks, ctx)
    _check_ks(ref.profile_like(rng, n, m), ks, ctx)


# ---- 2. many candidate tiles -------------------------------------------------

def test_many_tiles_and_ranges_compose(ctx):
    q, c, _, _ = _tile()
    n, m, k = 20_000, 64, 15
    assert n // c > 100 and n % c != 0
    x = np.random.default_rng(5).random((n, m))
    mid = (n // (2 * q)) * q
    ranges = [(3, 3 + q), (mid + 5, mid + 5 + q), (n - q, n)]
    assert all(lo % q != 0 and hi - lo == q for lo, hi in ranges)
    assert ranges[0][0] < q and ranges[2][1] == n  # the first tile, a middle one, the last (partial) one
    dev = _lib.DevBuf.from_numpy(ctx, x)
    try:
        whole = engine.knn_rows(dev, k, ctx=ctx)  # every query tile; candidates in hundreds of tiles
        for lo, hi in ranges:
            got = engine.knn_rows(dev, k, lo, hi, ctx=ctx)
            _same(got, ref.knn(x, k, lo, hi))
            _same(got, (whole[0][lo:hi], whole[1][lo:hi]))
        empty = engine.knn_rows(dev, k, mid, mid, ctx=ctx)
        assert empty[0].shape == (0, k) and empty[1].shape == (0, k)
        # the pieces side by side are the call over their union
        lo, hi = ranges[1]
        a = engine.knn_rows(dev, k, lo, lo + 7, ctx=ctx)
        b = engine.knn_rows(dev, k, lo + 7, hi, ctx=ctx)
        _same((np.concatenate([a[0], empty[0], b[0]]), np.concatenate([a[1], empty[1], b[1]])),
              (whole[0][lo:hi], whole[1][lo:hi]))
    finally:
        dev.close()


# ---- 3. ties -----------------------------------------------------------------

def test_ties_on_the_lattice(ctx):
    x = ref.tie_lattice()
    _, c, _, _ = _tile()
    assert len(x) > 2 * c  # ties across candidate tiles
    d2 = ref.d2_rows(x)
    srt = np.sort(d2, axis=1)
    assert np.count_nonzero(srt[:, 7] == srt[:, 8]) >= 100
    _check_ks(x, [8], ctx)


@pytest.mark.parametrize("copies", ["fewer", "more"])
def test_duplicate_rows_across_tiles(ctx, copies):
    _, c, _, _ = _tile()
    n, m, k = 2 * c + 40, 5, 8
    x = np.random.default_rng(9).random((n, m))
    at = [4, c + 9, 2 * c + 30] if copies == "fewer" else \
        [4, 11, 50, c - 1, c, c + 9, c + 77, 2 * c - 1, 2 * c, 2 * c + 30, 2 * c + 39]
    assert {i // c for i in at} == {0, 1, 2} and (len(at) < k if copies == "fewer" else len(at) > k)
    x[at] = x[at[0]]
    idx, dist = ref.knn(x, k)
    if copies == "fewer":
        assert all(idx[i, :len(at)].tolist() == at and dist[i, len(at) - 1] == 0 < dist[i, len(at)] for i in at)
    else:  # the last copies' own indices are not in their lists: self is no special case
        assert all(idx[i].tolist() == at[:k] for i in at) and at[-1] not in idx[at[-1]]
    _same(engine.knn_rows(x, k, ctx=ctx), (idx, dist))


def test_infinite_d2_ties_by_index(ctx):
    _, c, _, k_max = _tile()
    n, m, k = c + 30, 3, k_max
    x = np.random.default_rng(13).random((n, m))
    big = np.flatnonzero(np.arange(n) % 4 != 0)
    x[big, 0] = 1e160  # finite, but its square is not
    idx, dist = ref.knn(x, k)
    small = np.flatnonzero(np.arange(n) % 4 == 0)
    assert len(small) < k and np.isfinite(x).all()
    for i in small[[0, -1]]:  # finite neighbours first, then +inf in index order, from both tiles' candidates
        tail = idx[i, len(small):]
        assert np.isinf(dist[i, len(small):]).all() and np.isfinite(dist[i, :len(small)]).all()
        assert tail.tolist() == big[:len(tail)].tolist()
    assert big[-1] >= c
    _same(engine.knn_rows(x, k, ctx=ctx), (idx, dist))


def test_underflowing_and_subnormal_d2(ctx):
    _, c, _, _ = _tile()
    n, k = c + 9, 15
    rng = np.random.default_rng(17)
    x = np.stack([rng.integers(0, 4, n) * 3e-162, rng.integers(0, 3, n) * 1e-200], axis=1)
    d2 = ref.d2_rows(x)
    tiny = np.finfo(np.float64).tiny
    differ = (x[:, None, :] != x[None, :, :]).any(axis=2)
    assert np.count_nonzero((d2 == 0) & differ) > n  # squares of 1e-200 underflow to zero
    assert np.count_nonzero((d2 > 0) & (d2 < tiny)) > n  # (3e-162)^2 is subnormal
    idx, dist = ref.knn(x, k)
    assert (np.take_along_axis(d2, idx.astype(np.int64), 1) < tiny).any(axis=1).all()
    _same(engine.knn_rows(x, k, ctx=ctx), (idx, dist))


# ---- 4. row stride -----------------------------------------------------------

def test_row_stride_padding_is_never_read(ctx):
    q, _, p, _ = _tile()
    n, m, k = q + 5, p + 1, 15
    wide = np.full((n, m + 3), np.nan)
    wide[:, :m] = np.random.default_rng(21).random((n, m))
    x = wide[:, :m]
    assert engine._knn_source(x)[4] == m + 3 and np.isnan(wide[:, m:]).all()
    want = ref.knn(np.ascontiguousarray(x), k)
    assert np.isfinite(want[1]).all()
    _same(engine.knn_rows(x, k, ctx=ctx), want)
    # the same with the padded matrix on the device
    dev = _lib.DevBuf.from_numpy(ctx, wide)
    try:
        idx, dist = np.empty((n, k), np.int32), np.empty((n, k), np.float64)
        _lib.call("karma_knn_rows", ctx.h, ctypes.c_void_p(dev.ptr), n, m, m + 3, 1, 0, n, k, _lib.ptr(idx),
                  _lib.ptr(dist), 0)
        _same((idx, dist), want)
    finally:
        dev.close()


# ---- 5. pointer locations ----------------------------------------------------

def test_host_and_device_pointers_agree(ctx):
    q, c, _, _ = _tile()
    n, m, k = q + c + 3, 33, 15
    x = ref.profile_like(np.random.default_rng(23), n, m)
    want = ref.knn(x, k, 2, n - 1)
    dev = _lib.DevBuf.from_numpy(ctx, x)
    try:
        for src in (x, dev):
            _same(engine.knn_rows(src, k, 2, n - 1, ctx=ctx), want)
            di, dd = engine.knn_rows(src, k, 2, n - 1, ctx=ctx, out_device=True)
            assert isinstance(di, _lib.DevBuf) and isinstance(dd, _lib.DevBuf)
            _same((di.numpy(), dd.numpy()), want)
            di.close()
            dd.close()
    finally:
        dev.close()


# ---- 6. errors through the library -------------------------------------------

def test_argument_errors_and_messages(ctx):
    n, m, k = 10, 4, 3
    x = np.random.default_rng(29).random((n, m))
    idx, dist = np.full((n, k), -7, np.int32), np.full((n, k), -7.0)
    px, pi, pd = _lib.ptr(x), _lib.ptr(idx), _lib.ptr(dist)

    def call(x=px, n=n, m=m, ld=m, lo=0, hi=n, k=k, idx=pi, dist=pd):
        _lib.call("karma_knn_rows", ctx.h, x, n, m, ld, 0, lo, hi, k, idx, dist, 0)

    cases = [(dict(x=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(dist=None), "null pointer"),
             (dict(k=0), "1 <= k <= min(n, 64)"), (dict(k=n + 1), "1 <= k <= min(n, 64)"),
             (dict(n=1000, hi=1, k=65), "1 <= k <= min(n, 64)"),
             (dict(ld=m - 1), "ld must be at least m"),
             (dict(lo=-1), "0 <= row_lo <= row_hi <= n"), (dict(lo=5, hi=4), "0 <= row_lo <= row_hi <= n"),
             (dict(hi=n + 1), "0 <= row_lo <= row_hi <= n"),
             (dict(n=-1, hi=0), "must not be negative"), (dict(n=1 << 31, hi=1), "n < 2^31"),
             (dict(n=1 << 20, ld=1 << 40, hi=1), "byte size overflows"),
             (dict(x=ctypes.c_void_p(x.ctypes.data + 4)), "8-byte aligned")]
    for kw, text in cases:
        with pytest.raises(_lib.KarmaError) as e:
            call(**kw)
        assert e.value.code == _lib.KARMA_ERR_ARG and text in str(e.value), (kw, str(e.value))
    assert (idx == -7).all() and (dist == -7.0).all()  # nothing was written
    # nothing to do is no error, whatever else is passed
    call(lo=4, hi=4, k=0, idx=None, dist=None)
    call(n=0, hi=0, x=None, k=99)
    assert (idx == -7).all()
    call()
    _same((idx, dist), ref.knn(x, k))


# ---- 7. the public boundary --------------------------------------------------

def _seqs(seed=41, n=700):
    blob, offs, _ = engine.synth_contigs(seed, n, 30, 900, 200)
    return OrderedDict((f">ctg{i}", bytes(blob[offs[i]:offs[i + 1]]).decode()) for i in range(n))


@pytest.fixture(scope="module")
def contigs():
    """700 synthetic contigs, their host profile and the model's 15-NN of it
    (two model calls of half the rows each)."""
    seqs = _seqs()
    host = KmerClustering(seqs, "/tmp", "5p6", 4)._KmerClustering__calc_kmer_profile()
    half = len(host) // 2
    a, b = ref.knn(host, 15, 0, half), ref.knn(host, 15, half, len(host))
    want = (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))
    for arr in (host,) + want:
        arr.setflags(write=False)
    return seqs, host, want


def test_device_profile_knn_and_kmer_knn(contigs):
    seqs, host, want = contigs
    assert host.shape[0] == 700 and host.shape[1] > 1000
    dev = KmerClustering(seqs, "/tmp", "5p6", 4).calc_kmer_profile_device()
    _same(dev.knn(15), want)
    _same(dev.knn(15, 100, 231), (want[0][100:231], want[1][100:231]))
    dev.close()
    with pytest.raises(ValueError):
        dev.knn(15)
    kc = KmerClustering(seqs, "/tmp", "5p6", 4)
    prof, idx, dist = kc.kmer_knn(15)
    assert np.array_equal(prof.view(U64), host.view(U64)) and kc.kmers and kc.sorted_kmer_set == []
    _same((idx, dist), want)


def _stand_ins(monkeypatch, with_knn_parameter):
    """umap and hdbscan stand-ins in sys.modules; returns the list of UMAP calls."""
    calls = []

    class UMAPNew:
        def __init__(self, n_neighbors=15, n_components=2, min_dist=0.1, random_state=None,
                     precomputed_knn=(None, None, None)):
            self.kw = dict(n_neighbors=n_neighbors, n_components=n_components, min_dist=min_dist,
                           random_state=random_state, precomputed_knn=precomputed_knn)

        def fit_transform(self, X):
            calls.append((self.kw, X))
            return np.asarray(X)[:, :self.kw["n_components"]].copy()

    class UMAPOld:
        def __init__(self, n_neighbors=15, n_components=2, min_dist=0.1, random_state=None):
            self.kw = dict(n_neighbors=n_neighbors, n_components=n_components, min_dist=min_dist,
                           random_state=random_state)

        fit_transform = UMAPNew.fit_transform

    class HDBSCAN:
        def __init__(self, min_cluster_size=5, allow_single_cluster=False):
            pass

        def fit(self, reduced):
            self.labels_ = (np.arange(len(reduced)) % 4) - 1
            self.probabilities_ = np.linspace(0.0, 1.0, len(reduced))
            return self

    monkeypatch.setitem(sys.modules, "umap", types.SimpleNamespace(UMAP=UMAPNew if with_knn_parameter else UMAPOld))
    monkeypatch.setitem(sys.modules, "hdbscan", types.SimpleNamespace(HDBSCAN=HDBSCAN))
    return calls


def _run(seqs, out_dir, **kw):
    out_dir.mkdir()
    kc = KmerClustering(seqs, str(out_dir), "5p6", 4)
    kc.run(15, 2, 0.1, 42, 5, **kw)
    return (out_dir / "cluster.txt").read_text(), (out_dir / "eval.txt").read_text()


def test_run_hands_the_graph_to_umap(contigs, monkeypatch, tmp_path):
    seqs, host, want = contigs
    warnings = []
    monkeypatch.setattr(kmer_mod.logger, "warning", lambda msg, *a: warnings.append(msg))

    calls = _stand_ins(monkeypatch, with_knn_parameter=True)
    before = _run(seqs, tmp_path / "default")  # the default passes no such keyword
    assert len(calls) == 1 and calls[0][0]["precomputed_knn"] == (None, None, None)
    assert np.array_equal(calls[0][1].view(U64), host.view(U64))

    files = _run(seqs, tmp_path / "knn", device_knn=True)
    kw, X = calls[1]
    assert isinstance(kw["precomputed_knn"], tuple) and len(kw["precomputed_knn"]) == 2
    _same(kw["precomputed_knn"], want)
    assert np.array_equal(X.view(U64), host.view(U64))
    assert {k: kw[k] for k in ("n_neighbors", "n_components", "min_dist", "random_state")} == \
        {k: calls[0][0][k] for k in ("n_neighbors", "n_components", "min_dist", "random_state")}
    assert files == before and files[0].count("\n") == 4 and not warnings

    calls = _stand_ins(monkeypatch, with_knn_parameter=False)
    old = _run(seqs, tmp_path / "old", device_knn=True)  # an UMAP without the parameter: the existing call
    assert len(calls) == 1 and "precomputed_knn" not in calls[0][0] and len(warnings) == 1
    assert np.array_equal(calls[0][1].view(U64), host.view(U64)) and old == before
    _run(seqs, tmp_path / "old_default")
    assert len(calls) == 2 and len(warnings) == 1
