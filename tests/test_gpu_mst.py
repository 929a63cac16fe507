"""karma_mreach_mst on the GPU against the numpy model (tests/mst_reference.py):
edges equal, weights and core distances bit for bit, exactly n - 1 edges.
Shapes sit on karma_mst_tile()'s edges."""
import numpy as np
import pytest

import mst_reference as ref
from karma_amd import _lib, engine

pytestmark = pytest.mark.gpu

U64 = np.uint64


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def _check(x, min_samples, ctx, src=None):
    x = np.asarray(x, np.float64)
    n = len(x)
    wa, wb, ww, wc = ref.mreach_mst(x, min_samples)
    a, b, w, core = engine.mreach_mst(x if src is None else src, min_samples, ctx=ctx)
    assert a.dtype == np.int32 and b.dtype == np.int32 and w.dtype == np.float64 and core.dtype == np.float64
    assert a.shape == b.shape == w.shape == (n - 1,) and core.shape == (n,)
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    assert np.array_equal(w.view(U64), ww.view(U64))
    assert np.array_equal(core.view(U64), wc.view(U64))
    return a, b, w, core


def _resolve(name):
    q, c, p, _ = _lib.mst_tile()
    named = {"q-1": q - 1, "q": q, "q+1": q + 1, "c+1": c + 1, "2c+q+1": 2 * c + q + 1,
             "p-1": p - 1, "p": p, "p+1": p + 1}
    return named[name] if name in named else int(name)


# ---- 1. tile edges -----------------------------------------------------------

@pytest.mark.parametrize("n_at", ["1", "2", "3", "q-1", "q", "q+1", "c+1", "2c+q+1"])
def test_rows_on_tile_edges(ctx, n_at):
    n = _resolve(n_at)
    x = ref.blobs(np.random.default_rng(100 + n), n, 10, 4, 0.3)
    _check(x, min(n, 5), ctx)


@pytest.mark.parametrize("m_at", ["0", "1", "2", "p-1", "p", "p+1"])
def test_columns_on_panel_edges(ctx, m_at):
    m, n = _resolve(m_at), _resolve("q+1")
    x = np.random.default_rng(200 + m).normal(size=(n, m))
    _check(x, 4, ctx)


@pytest.mark.parametrize("min_samples", [1, 2, 15, 64])
def test_min_samples(ctx, min_samples):
    x = ref.blobs(np.random.default_rng(7), 200, 10, 5, 0.2)
    _, _, _, core = _check(x, min_samples, ctx)
    if min_samples == 1:
        assert (core == 0).all()  # the plain Euclidean tree


def test_min_samples_of_every_row(ctx):
    # every core2 is a row's largest d2: almost every key ties on its weight
    x = np.random.default_rng(8).integers(0, 4, (50, 3)).astype(np.float64)
    _check(x, 50, ctx)


# ---- 2. where the matrix lies ------------------------------------------------

def test_row_stride(ctx):
    q = _resolve("q")
    wide = np.random.default_rng(9).normal(size=(q + 7, 16))
    view = wide[:, :10]
    assert engine._knn_source(view)[4] == 16
    _check(np.ascontiguousarray(view), 5, ctx, src=view)


def test_device_resident_input(ctx):
    x = ref.blobs(np.random.default_rng(10), _resolve("c+1"), 10, 3, 0.2)
    dev = _lib.DevBuf.from_numpy(ctx, x)
    try:
        _check(x, 5, ctx, src=dev)
    finally:
        dev.close()


# ---- 3. ties -----------------------------------------------------------------

def test_identical_rows_make_the_star_of_row_0(ctx):
    n = _resolve("q+1")
    a, b, w, core = _check(np.full((n, 3), 0.5), 3, ctx)
    assert (a == 0).all() and np.array_equal(b, np.arange(1, n)) and (w == 0).all() and (core == 0).all()


@pytest.mark.parametrize("copies", [2, 3])
def test_duplicated_rows(ctx, copies):
    rng = np.random.default_rng(11)
    x = np.tile(rng.normal(size=(70, 4)), (copies, 1))[rng.permutation(70 * copies)]
    for min_samples in (1, copies, copies + 1):
        _check(x, min_samples, ctx)


def test_integer_grid(ctx):
    grid = np.stack(np.meshgrid(np.arange(17.0), np.arange(11.0)), -1).reshape(-1, 2)
    for min_samples in (1, 4, 5):
        _check(grid, min_samples, ctx)


# ---- 4. rounds ---------------------------------------------------------------

def _check_counting_rounds(x, min_samples, ctx):
    """_check with the library's timing table on: (result, launches per kernel name)."""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        got = _check(x, min_samples, ctx)
        table = ctx.timing_read()
    finally:
        ctx.timing(False)
    return got, {name: launches for name, (_, launches) in table.items()}


def test_components_double_every_round(ctx):
    i = np.arange(1, 1024)
    gaps = 1.0 + np.log2(i & -i)  # the gap after point i - 1 grows with the trailing zeros of i
    x = np.concatenate([[0.0], np.cumsum(gaps)])[:, None]
    (a, b, _, _), launches = _check_counting_rounds(x, 1, ctx)
    assert np.array_equal(np.sort(a), np.arange(1023)) and (b == a + 1).all()
    # pairs, then pairs of pairs, ...: every one of the ceil(log2 n) rounds the bound allows is needed
    assert launches["mst_nearest"] == 10 and launches["mst_reduce"] == 20 and launches["mst_core"] == 1
    assert launches["mst_hook"] >= 2 * 10 and launches["profile_knn_block"] == 1


def test_one_chain_in_the_first_round(ctx):
    gaps = 1.0 + np.arange(1023) / 1024.0  # strictly increasing: every point's nearest is the one before it
    x = np.concatenate([[0.0], np.cumsum(gaps)])[:, None]
    (a, b, _, _), launches = _check_counting_rounds(x, 1, ctx)
    assert np.array_equal(a, np.arange(1023)) and (b == a + 1).all()
    # one round hooks all 1024 components into one chain: 1 hook, ceil(log2 1024) jumps, 1 relabel
    assert launches["mst_nearest"] == 1 and launches["mst_hook"] == 1 + 10 + 1


def test_two_far_blobs_of_unequal_size(ctx):
    # late rounds: whole tiles of the first blob share one component (the tiles a block may skip)
    q, c, _, _ = _lib.mst_tile()
    rng = np.random.default_rng(12)
    x = np.vstack([rng.normal(size=(2 * c + 40, 10)), 1e3 + rng.normal(size=(q - 40 + 5, 10))])
    a, b, w, _ = _check(x, 5, ctx)
    assert w[-1] > 100 * w[-2] and a[-1] < 2 * c + 40 <= b[-1]


def test_many_tiles_in_uneven_slices(ctx):
    # 25 candidate tiles and 25 query blocks: on a device that holds 512 blocks the tiles are dealt to 20
    # slices of one or two tiles each, and shuffled rows keep every tile mixed until the last rounds
    _, c, _, _ = _lib.mst_tile()
    rng = np.random.default_rng(14)
    n = 24 * c + 5
    x = ref.blobs(rng, n, 3, 7, 0.3)[rng.permutation(n)]
    _check(x, 5, ctx)


def test_overflowing_d2_still_spans(ctx):
    rng = np.random.default_rng(13)
    x = np.vstack([rng.normal(size=(70, 2)), 1e200 * (1.0 + rng.random((60, 2)))])
    a, b, w, _ = _check(x, 2, ctx)
    assert np.isinf(w).any() and np.isfinite(w[0])
