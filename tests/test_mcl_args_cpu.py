"""The MCL entries without a device: engine's own argument checks, the ABI's
declaration of the entries, the library's argument errors with no context
(found before a device is looked for), and the checks and batch arithmetic
(csrc/mcl_args.h) in a stand-alone program built with AddressSanitizer + UBSan.
The kernels themselves: tests/test_gpu_mcl.py."""
import ctypes
import os
import re
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


GRAPH = (np.array([0, 1, 2, 2], np.int64), np.array([1, 0], np.uint32), np.array([1.0, 1.0]))


def test_engine_argument_errors():
    ctx = NoContext()
    for kw in (dict(resource=1), dict(resource=33), dict(inflation=1.0), dict(inflation=16.5), dict(cutoff=0.0),
               dict(cutoff=0.6), dict(eps=-1.0), dict(eps=float("nan")), dict(max_iter=0), dict(cand_cap=-1),
               dict(cand_cap=2 ** 32)):
        with pytest.raises(ValueError):
            engine.mcl(*GRAPH, ctx=ctx, **kw)
    with pytest.raises(ValueError):
        engine.mcl(np.array([0], np.int64), GRAPH[1], GRAPH[2], ctx=ctx)  # n = 0
    with pytest.raises(ValueError):
        engine.mcl(GRAPH[0], GRAPH[1], GRAPH[2][:1], ctx=ctx)
    with pytest.raises(ValueError):
        engine.mcl_clusters(np.array([0], np.int64), np.zeros(0, np.uint32), np.zeros(0))
    with pytest.raises(ValueError):
        engine.mcl_clusters(np.array([0, 2], np.int64), np.zeros(1, np.uint32), np.zeros(1))


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_mcl", "karma_adj_mcl", "karma_mcl_clusters", "karma_mcl_tile"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_mcl.argtypes) == 20 and len(lib.karma_adj_mcl.argtypes) == 15
    assert len(lib.karma_mcl_clusters.argtypes) == 6
    tile = _lib.mcl_tile()  # host only: no device needed
    assert tile.COLS * tile.LANES4 == 256 and tile.LANES4 == 16 and tile.LANES8 == 64 and tile.CAND_CAP >= 1 << 16
    assert lib.karma_mcl_tile(None, 4) == _lib.KARMA_ERR_ARG
    assert b"karma_mcl_tile" in lib.karma_last_error()
    assert _lib.KARMA_MCL_GENERAL == 1


def test_header_declares_the_entries_and_the_contract():
    text = open(os.path.join(REPO, "include", "karma.h")).read()
    for decl in (r"int karma_mcl\(karma_ctx\* ctx, int64_t n, const int64_t\* off, const uint32_t\* nbr",
                 r"int karma_adj_mcl\(karma_adj\* g, double inflation, int resource",
                 r"int karma_mcl_clusters\(int64_t n, const int64_t\* colptr",
                 r"int karma_mcl_tile\(int\* v, int n\)", r"#define KARMA_MCL_GENERAL 1"):
        assert re.search(decl, text), decl
    for phrase in ("equality with the binary's", "every z > 0", "A uniform clique converges in one iteration",
                   "does not depend on block shape", "mcl_start", "mcl_expand", "mcl_iter"):
        assert phrase in text, phrase


def test_argument_errors_come_before_a_device():
    lib = _lib.load()
    off, nbr, w = GRAPH
    n, R = 3, 4
    colptr, rows, vals = np.full(n + 1, -7, np.int64), np.full(n * R, 7, np.uint32), np.full(n * R, -7.0)
    it, chaos = ctypes.c_int32(-7), ctypes.c_double(-7.0)

    def rc(ctx=None, n=n, off=off, nbr=nbr, w=w, inflation=2.0, resource=R, cutoff=1 / 4000, eps=1e-3, max_iter=10,
           flags=0, cand_cap=0, colptr=_lib.ptr(colptr), rows=_lib.ptr(rows), vals=_lib.ptr(vals), cap=n * R,
           it=ctypes.byref(it), chaos=ctypes.byref(chaos)):
        return lib.karma_mcl(ctx, n, _lib.ptr(off) if off is not None else None,
                             _lib.ptr(nbr) if nbr is not None else None, _lib.ptr(w) if w is not None else None, 0,
                             inflation, resource, cutoff, eps, max_iter, flags, cand_cap, colptr, rows, vals, cap, it,
                             chaos, 0)

    def message():
        return lib.karma_last_error().decode()

    # a null context is the last thing found: everything else is checked first
    assert rc() == _lib.KARMA_ERR_ARG and "null context" in message()
    for kw, word in ((dict(n=0), "n <"), (dict(off=None), "null"), (dict(colptr=None), "null"),
                     (dict(rows=None), "null"), (dict(vals=None), "null"), (dict(it=None), "null"),
                     (dict(chaos=None), "null"), (dict(resource=1), "resource"), (dict(resource=33), "resource"),
                     (dict(inflation=1.0), "inflation"), (dict(inflation=17.0), "inflation"),
                     (dict(cutoff=2.0 ** -41), "cutoff"), (dict(cutoff=0.51), "cutoff"), (dict(eps=-1.0), "eps"),
                     (dict(max_iter=0), "max_iter"), (dict(flags=2), "flag"), (dict(cand_cap=-1), "cand_cap"),
                     (dict(cap=n * R - 1), "n * resource"),
                     (dict(off=np.array([1, 1, 2, 2], np.int64)), "off"),
                     (dict(off=np.array([0, 2, 1, 2], np.int64)), "off"),
                     (dict(off=np.array([0, 1, 3, 2], np.int64)), "off"),
                     (dict(nbr=np.array([1, 3], np.uint32)), "outside"),
                     (dict(w=np.array([1.0, 0.0])), "weights"), (dict(w=np.array([1.0, np.inf])), "weights"),
                     (dict(w=np.array([np.nan, 1.0])), "weights"),
                     (dict(off=np.array([0, 2, 2, 2], np.int64), nbr=np.array([1, 1], np.uint32)), "twice"),
                     (dict(colptr=ctypes.c_void_p(colptr.ctypes.data + 4)), "aligned"),
                     (dict(rows=ctypes.c_void_p(rows.ctypes.data + 1)), "aligned")):
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert word in message() and "null context" not in message(), (kw, message())
    # nothing was written
    assert (colptr == -7).all() and (rows == 7).all() and (vals == -7.0).all()
    assert it.value == -7 and chaos.value == -7.0
    # karma_adj_mcl without a graph
    assert lib.karma_adj_mcl(None, 2.0, 4, 1 / 4000, 1e-3, 10, 0, 0, _lib.ptr(colptr), _lib.ptr(rows), _lib.ptr(vals),
                             n * R, ctypes.byref(it), ctypes.byref(chaos), 0) == _lib.KARMA_ERR_ARG


def test_args_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "mcl_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "mcl_args_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_args_header_is_host_only():
    text = open(os.path.join(CSRC, "mcl_args.h")).read()
    assert "#include <hip" not in text and "karma_internal.h\"" not in text
