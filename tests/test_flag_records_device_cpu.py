"""engine.flag_records_device / FlaggedRecords without a device: the argument
checks that run before anything reaches the library, the ABI's declaration of
karma_records_flag, and the entry's own argument and overlap checks
(csrc/flag_args.h, a host-only header) in a stand-alone program built with
AddressSanitizer + UBSan.  The kernels themselves: tests/test_gpu_flag_records.py."""
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


def test_shape_and_dtype_errors():
    ctx = NoContext()
    for bad in (np.zeros((3, 3), np.uint32), np.zeros(6, np.uint32), np.zeros((2, 2, 2), np.uint32),
                [1, 2, 3], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            engine.flag_records_device(bad, ctx=ctx)
    for bad in (np.zeros((3, 2), np.float64), np.zeros((3, 2), bool), [["a", "b"]], [[1.0, 2.0]]):
        with pytest.raises(TypeError):
            engine.flag_records_device(bad, ctx=ctx)
    for bad in (np.array([[0, -1]], np.int64), np.array([[1 << 32, 0]], np.int64), [[0, 1 << 40]]):
        with pytest.raises(ValueError):
            engine.flag_records_device(bad, ctx=ctx)


def test_records_and_device_ptr_exclude_each_other():
    ctx = NoContext()
    with pytest.raises(ValueError):
        engine.flag_records_device(ctx=ctx)
    with pytest.raises(ValueError):
        engine.flag_records_device(np.zeros((1, 2), np.uint32), device_ptr=4096, n_records=1, ctx=ctx)
    with pytest.raises(ValueError):
        engine.flag_records_device(device_ptr=4096, ctx=ctx)  # device_ptr without n_records
    with pytest.raises(ValueError):
        engine.flag_records_device(device_ptr=4096, n_records=-1, ctx=ctx)
    with pytest.raises(ValueError):
        engine.flag_records_device(np.zeros((1, 2), np.uint32), n_records=1, ctx=ctx)
    with pytest.raises(TypeError):
        engine.flag_records_device(np.zeros((1, 2), np.uint32), 4096, 1)  # keyword-only after records


def test_pairs_array_accepts_what_flag_records_accepts():
    rec = np.array([[4, 2], [9, 1], [9, 3]], np.uint32)
    for form in (rec, rec.tolist(), rec.astype(np.int64), np.asfortranarray(rec), np.repeat(rec, 2, axis=0)[::2]):
        a = engine._pairs_array(form)
        assert a.dtype == np.uint32 and a.flags.c_contiguous and np.array_equal(a, rec)
    for empty in ([], np.zeros((0, 2), np.uint32), np.zeros(0, np.int64)):
        assert engine._pairs_array(empty).shape == (0, 2)


def test_flagged_records_holds_what_it_is_given():
    class Buf:
        ptr = 0x1000
        closed = False

        def numpy(self):
            return np.arange(8, dtype=np.uint32)

        def close(self):
            self.closed = True

    buf = Buf()
    fr = engine.FlaggedRecords(None, buf, 5, 3)
    assert (fr.ptr, fr.n_records, fr.n_reads) == (0x1000, 5, 3)
    assert fr.to_host().tolist() == [0, 1, 2, 3, 4]
    fr.close()
    fr.close()
    assert buf.closed


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_records_flag", "karma_records_flag_tile", "karma_classify_launches"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_records_flag.argtypes) == 8
    per_thread, per_wave, per_block = _lib.flag_tile()  # host only: no device needed
    assert per_thread * 4 == 16 and per_wave == 64 * per_thread and per_block % per_wave == 0
    p, f = ctypes.c_uint64(1), ctypes.c_uint64(1)
    assert lib.karma_classify_launches(ctypes.byref(p), ctypes.byref(f)) == 0
    assert lib.karma_classify_launches(None, None) == _lib.KARMA_ERR_ARG


def test_argument_and_overlap_checks_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "flag_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "flag_args_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_flag_args_header_is_host_only():
    hdr = open(os.path.join(CSRC, "flag_args.h")).read()
    assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
