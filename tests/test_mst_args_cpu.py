"""engine.mreach_mst / engine.hdbscan without a device: the argument checks that
run before anything reaches a context, the ABI's declaration of the entries,
karma_mreach_mst's own argument errors with no context, and its checks
(csrc/mst_args.h, a host-only header) in a stand-alone program built with
AddressSanitizer + UBSan.  The kernels themselves: tests/test_gpu_mst.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from karma_amd import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


class NoContext:
    """Stands where a context would: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the argument check must come before the library is reached")


def test_matrix_shape_and_dtype_errors():
    ctx = NoContext()
    for bad in (np.zeros(6), np.zeros((2, 2, 2)), 3.0, np.zeros((0, 3))):
        with pytest.raises(ValueError):
            engine.mreach_mst(bad, 1, ctx=ctx)
        with pytest.raises(ValueError):
            engine.hdbscan(bad, 2, 1, ctx=ctx)
    for bad in (np.zeros((3, 2), np.float32), np.zeros((3, 2), np.int64), [[1, 2], [3, 4]]):
        with pytest.raises(TypeError):
            engine.mreach_mst(bad, 1, ctx=ctx)
        with pytest.raises(TypeError):
            engine.hdbscan(bad, 2, ctx=ctx)


def test_min_samples_and_min_cluster_size_errors():
    ctx = NoContext()
    x = np.zeros((100, 3))
    k_max = _lib.knn_tile()[3]
    assert k_max == 64
    for min_samples in (0, -1, 101, k_max + 1):
        with pytest.raises(ValueError):
            engine.mreach_mst(x, min_samples, ctx=ctx)
        with pytest.raises(ValueError):
            engine.hdbscan(x, 5, min_samples, ctx=ctx)
    with pytest.raises(ValueError):
        engine.mreach_mst(np.zeros((5, 3)), 6, ctx=ctx)  # min_samples > n
    with pytest.raises(ValueError):
        engine.hdbscan(np.zeros((4, 3)), ctx=ctx)  # min_samples = min_cluster_size = 5 > n
    with pytest.raises(ValueError):
        engine.hdbscan(x, 65, ctx=ctx)  # min_samples = min_cluster_size > 64
    for size in (1, 0, -2):
        with pytest.raises(ValueError):
            engine.hdbscan(x, size, 3, ctx=ctx)


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_mreach_mst", "karma_mst_tile", "karma_hdbscan_tree"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_mreach_mst.argtypes) == 12
    q, c, panel, rounds = _lib.mst_tile()  # host only: no device needed
    assert (q, c, panel) == _lib.knn_tile()[:3] and rounds == 31
    assert lib.karma_mst_tile(None, None, None, None) == _lib.KARMA_ERR_ARG
    assert b"karma_mst_tile" in lib.karma_last_error()


def test_library_argument_errors_come_before_a_device():
    lib = _lib.load()
    n, m = 4, 2
    x = np.zeros((n, m))
    a, b = np.full(n - 1, -7, np.int32), np.full(n - 1, -7, np.int32)
    w, core = np.full(n - 1, -7.0), np.full(n, -7.0)

    def rc(ctx=None, x=_lib.ptr(x), n=n, m=m, ld=m, min_samples=2, a=_lib.ptr(a), b=_lib.ptr(b), w=_lib.ptr(w),
           core=_lib.ptr(core)):
        return lib.karma_mreach_mst(ctx, x, n, m, ld, 0, min_samples, a, b, w, core, 0)

    cases = [(dict(x=None), b"null pointer"), (dict(a=None), b"null pointer"), (dict(b=None), b"null pointer"),
             (dict(w=None), b"null pointer"), (dict(core=None), b"null pointer"),
             (dict(min_samples=0), b"1 <= min_samples <= min(n, 64)"),
             (dict(min_samples=n + 1), b"1 <= min_samples <= min(n, 64)"),
             (dict(n=1000, min_samples=65), b"1 <= min_samples <= min(n, 64)"),
             (dict(ld=m - 1), b"ld must be at least m"),
             (dict(n=0), b"1 <= n < 2^31"), (dict(n=1 << 31), b"1 <= n < 2^31"), (dict(m=-1), b"m >= 0"),
             (dict(n=1 << 20, ld=1 << 40), b"byte size overflows"),
             (dict(x=ctypes.c_void_p(x.ctypes.data + 4)), b"8-byte aligned"),
             (dict(a=ctypes.c_void_p(a.ctypes.data + 2)), b"4-byte aligned"),
             (dict(), b"null context")]  # every argument in order: only the context is missing
    for kw, text in cases:
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert text in lib.karma_last_error(), (kw, lib.karma_last_error())
    assert (a == -7).all() and (b == -7).all() and (w == -7.0).all() and (core == -7.0).all()


def test_argument_checks_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "mst_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "mst_args_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_mst_args_header_is_host_only():
    hdr = open(os.path.join(CSRC, "mst_args.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
