"""engine.knn_rows / DeviceProfile.knn without a device: the argument checks
that run before anything reaches the library, the ABI's declaration of the
entries, and karma_knn_rows' own argument checks (csrc/knn_args.h, a host-only
header) in a stand-alone program built with AddressSanitizer + UBSan.  The
kernel itself: tests/test_gpu_knn.py."""
import os
import subprocess

import numpy as np
import pytest

from karma_amd import _lib, engine
from karma_amd.device_profile import DeviceProfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")


class NoContext:
    """Stands where a context would: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the argument check must come before the library is reached")


def test_matrix_shape_and_dtype_errors():
    ctx = NoContext()
    for bad in (np.zeros(6), np.zeros((2, 2, 2)), 3.0):
        with pytest.raises(ValueError):
            engine.knn_rows(bad, 1, ctx=ctx)
    for bad in (np.zeros((3, 2), np.float32), np.zeros((3, 2), np.int64), [[1, 2], [3, 4]]):
        with pytest.raises(TypeError):
            engine.knn_rows(bad, 1, ctx=ctx)


def test_k_and_row_range_errors():
    ctx = NoContext()
    x = np.zeros((100, 3))
    k_max = _lib.knn_tile()[3]
    assert k_max >= 64
    for k in (0, -1, 101, k_max + 1):
        with pytest.raises(ValueError):
            engine.knn_rows(x, k, ctx=ctx)
    with pytest.raises(ValueError):
        engine.knn_rows(np.zeros((5, 3)), 6, ctx=ctx)  # k > n
    for lo, hi in ((-1, 5), (6, 5), (0, 101), (101, 101)):
        with pytest.raises(ValueError):
            engine.knn_rows(x, 3, lo, hi, ctx=ctx)


def test_source_keeps_a_row_stride_and_copies_the_rest():
    wide = np.arange(60, dtype=np.float64).reshape(6, 10)
    host, dptr, n, m, ld = engine._knn_source(wide[:, :7])
    assert dptr is None and (n, m, ld) == (6, 7, 10) and host.ctypes.data == wide.ctypes.data
    host, _, n, m, ld = engine._knn_source(wide[1:5, 2:9])
    assert (n, m, ld) == (4, 7, 10) and host.ctypes.data == wide.ctypes.data + 8 * 12
    for view in (wide.T, wide[:, ::2], wide[::-1], np.asfortranarray(wide)):
        host, _, n, m, ld = engine._knn_source(view)
        assert host.flags.c_contiguous and ld == m == view.shape[1] and np.array_equal(host, view)
    assert engine._knn_source(np.zeros((0, 4)))[2:] == (0, 4, 4)
    assert engine._knn_source(np.zeros((3, 0)))[2:] == (3, 0, 0)


def test_closed_profile_raises():
    class Buf:
        ptr = 0x1000

        def close(self):
            pass

    prof = DeviceProfile(NoContext(), Buf(), 4, 3, ["a", "b", "c"])
    prof.close()
    with pytest.raises(ValueError):
        prof.knn(2)
    with pytest.raises(ValueError):
        engine.knn_rows(prof, 2)


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_knn_rows", "karma_knn_tile"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_knn_rows.argtypes) == 12
    q, c, panel, k_max = _lib.knn_tile()  # host only: no device needed
    assert q > 0 and c > 0 and panel > 0 and k_max >= 64
    assert lib.karma_knn_tile(None, None, None, None) == _lib.KARMA_ERR_ARG
    # argument errors are reported before a device is looked for
    out_i, out_d = np.zeros(4, np.int32), np.zeros(4, np.float64)
    x = np.zeros((4, 2))
    rc = lib.karma_knn_rows(None, _lib.ptr(x), 4, 2, 2, 0, 0, 4, 1, _lib.ptr(out_i), _lib.ptr(out_d), 0)
    assert rc == _lib.KARMA_ERR_ARG


def test_argument_checks_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "knn_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "knn_args_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_knn_args_header_is_host_only():
    hdr = open(os.path.join(CSRC, "knn_args.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
