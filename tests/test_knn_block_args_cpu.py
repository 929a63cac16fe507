"""engine.KnnState / engine.knn_blocked / distributed.knn_sharded without a
device: the argument checks that run before anything reaches the library, the
ABI's declaration of the entries, and the library's own checks and split
arithmetic (csrc/knn_block_args.h, a host-only header) in a stand-alone program
built with AddressSanitizer + UBSan.  The kernels: tests/test_gpu_knn_block.py."""
import os
import subprocess

import numpy as np
import pytest

from karma_amd import _lib, distributed, engine
from karma_amd.comm import SoloComm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


class NoContext:
    """Stands where a context would: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the argument check must come before the library is reached")


def test_state_shape_errors():
    ctx = NoContext()
    k_max = _lib.knn_tile()[3]
    for k in (0, -1, k_max + 1):
        with pytest.raises(ValueError, match="1 <= k <="):
            engine.KnnState(ctx, 10, k)
    for nq in (-1, 1 << 31):
        with pytest.raises(ValueError, match="nq"):
            engine.KnnState(ctx, nq, 3)
    engine.KnnState(ctx, 10, k_max)  # nothing is allocated before the first update


def test_update_errors_come_before_the_library():
    ctx = NoContext()
    st = engine.KnnState(ctx, 5, 3)
    q, c = np.zeros((5, 4)), np.zeros((7, 4))
    with pytest.raises(ValueError, match="5 query rows"):
        st.update(np.zeros((6, 4)), c, 0)
    with pytest.raises(ValueError, match="same columns"):
        st.update(q, np.zeros((7, 3)), 0)
    with pytest.raises(ValueError, match="cand_base"):
        st.update(q, c, -1)
    with pytest.raises(ValueError, match="cand_base"):
        st.update(q, c, (1 << 31) - 1 - 6)  # the last index would be 2^31 - 1
    with pytest.raises(ValueError, match="cand_split"):
        st.update(q, c, 0, cand_split=-1)
    for bad in (np.zeros(5), np.zeros((5, 4, 1))):
        with pytest.raises(ValueError):
            st.update(bad, c, 0)
    for bad in (np.zeros((5, 4), np.float32), [[1, 2]] * 5):
        with pytest.raises(TypeError):
            st.update(bad, c, 0)
        with pytest.raises(TypeError):
            st.update(q, bad, 0)
    assert st.first and st.rows_seen == 0 and st.keys is None  # untouched by the failures
    with pytest.raises(ValueError, match="candidate rows offered"):
        st.finish()
    with pytest.raises(TypeError):
        st.merge((None, None))
    with pytest.raises(ValueError, match="differ"):
        st.merge(engine.KnnState(ctx, 5, 4))
    with pytest.raises(ValueError, match="itself"):
        st.merge(st)
    st.merge(engine.KnnState(ctx, 5, 3))  # an untouched state adds nothing, and reaches no library
    assert st.first and st.rows_seen == 0
    st.close()
    for use in (lambda: st.update(q, c, 0), st.finish, lambda: st.merge(engine.KnnState(ctx, 5, 3))):
        with pytest.raises(ValueError, match="closed"):
            use()


def test_state_counts_the_rows_it_was_given():
    st = engine.KnnState(NoContext(), 0, 3)  # no query rows: nothing reaches the library
    st.update(np.zeros((0, 4)), np.zeros((2, 4)), 0)
    with pytest.raises(ValueError, match="k = 3 with 2 rows"):
        st.finish()
    st.update(np.zeros((0, 4)), np.zeros((1, 4)), 2)
    idx, dist = st.finish()
    assert idx.shape == (0, 3) and idx.dtype == np.int32 and dist.shape == (0, 3) and dist.dtype == np.float64


def test_knn_blocked_errors():
    ctx = NoContext()
    x = np.zeros((20, 3))
    for bad in ([[1.0, 2.0]], None):
        with pytest.raises(TypeError):
            engine.knn_blocked(bad, 1, 4, ctx=ctx)
    with pytest.raises(TypeError):
        engine.knn_blocked(x.astype(np.float32), 1, 4, ctx=ctx)
    with pytest.raises(ValueError):
        engine.knn_blocked(np.zeros(20), 1, 4, ctx=ctx)
    for k in (0, 21, 65):
        with pytest.raises(ValueError, match="1 <= k <= min"):
            engine.knn_blocked(np.zeros((100, 3)) if k == 65 else x, k, 4, ctx=ctx)
    with pytest.raises(ValueError, match="block_rows"):
        engine.knn_blocked(x, 3, 0, ctx=ctx)


def test_knn_sharded_errors_come_before_any_collective():
    class NoComm:
        world, rank = 3, 1

        def __getattr__(self, name):
            raise AssertionError("no collective before the arguments are checked")

    ctx = NoContext()
    local = np.zeros((4, 2))
    for k in (0, 11, 65):
        with pytest.raises(ValueError, match="1 <= k <= min"):
            distributed.knn_sharded(NoComm(), ctx, local, [0, 3, 7, 1000 if k == 65 else 10], k)
    for bounds in ([0, 3, 7], [1, 3, 7, 10], [0, 7, 3, 10]):
        with pytest.raises(ValueError, match="bounds"):
            distributed.knn_sharded(NoComm(), ctx, local, bounds, 3)
    with pytest.raises(TypeError, match="on the device"):
        distributed.knn_sharded(NoComm(), ctx, local, [0, 3, 7, 10], 3)
    with pytest.raises(ValueError, match="1 <= k <= min"):
        distributed.knn_sharded(SoloComm(), ctx, local, [0, 4], 5)


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_knn_block", "karma_knn_merge", "karma_knn_finish", "karma_knn_block_split"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_knn_block.argtypes) == 17 and len(lib.karma_knn_merge.argtypes) == 8
    assert len(lib.karma_knn_finish.argtypes) == 9 and len(lib.karma_knn_block_split.argtypes) == 5
    # argument errors are reported before a device is looked for
    x = np.zeros((4, 2))
    keys, idx = np.zeros((4, 3), np.uint64), np.zeros((4, 3), np.int32)
    out_i, out_d = np.zeros((4, 3), np.int32), np.zeros((4, 3))
    p = _lib.ptr
    assert lib.karma_knn_block(None, p(x), 4, 2, 0, p(x), 4, 2, 0, 2, 0, 3, p(keys), p(idx), 0, 1, 0) == _lib.KARMA_ERR_ARG
    assert lib.karma_knn_merge(None, p(keys), p(idx), p(keys), p(idx), 4, 3, 0) == _lib.KARMA_ERR_ARG
    assert lib.karma_knn_finish(None, p(keys), p(idx), 4, 3, 0, p(out_i), p(out_d), 0) == _lib.KARMA_ERR_ARG
    # an explicit split is arithmetic alone: clamped to the candidate tiles and to 32
    c = _lib.knn_tile()[1]
    assert _lib.knn_block_split(None, 100, 3 * c, 1) == 1
    assert _lib.knn_block_split(None, 100, 3 * c - 1, 7) == 3
    assert _lib.knn_block_split(None, 100, 9 * c - 5, 7) == 7
    assert _lib.knn_block_split(None, 100, 9 * c - 5, 1000) == 9
    assert _lib.knn_block_split(None, 100, 1000 * c, 1000) == 32
    assert _lib.knn_block_split(None, 100, 0, 5) == 1
    with pytest.raises(_lib.KarmaError, match="cand_split must not be negative"):
        _lib.knn_block_split(None, 100, 100, -1)
    with pytest.raises(_lib.KarmaError, match="null context"):
        _lib.knn_block_split(None, 100, 100, 0)  # auto asks the device


def test_argument_checks_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "knn_block_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "knn_block_args_test")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_knn_block_args_header_is_host_only():
    hdr = open(os.path.join(CSRC, "knn_block_args.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
