"""The UMAP entries without a device: engine's own argument checks, the ABI's
declaration of the entries, the library's argument errors with no context, and
the checks and defined functions (csrc/umap_args.h, csrc/umap_math.h) in a
stand-alone program built with AddressSanitizer + UBSan.  The kernels
themselves: tests/test_gpu_umap.py."""
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


def test_engine_argument_errors():
    ctx = NoContext()
    idx, dist = np.zeros((5, 3), np.int32), np.zeros((5, 3))
    for bad_idx, bad_dist in ((np.zeros(5, np.int32), np.zeros(5)), (idx, np.zeros((5, 2))),
                              (np.zeros((5, 1), np.int32), np.zeros((5, 1))),  # k = 1: log2(k) is 0
                              (np.zeros((5, 6), np.int32), np.zeros((5, 6))),  # k > n
                              (np.zeros((1, 1), np.int32), np.zeros((1, 1))),
                              (np.zeros((100, 65), np.int32), np.zeros((100, 65)))):
        with pytest.raises(ValueError):
            engine.umap_graph(bad_idx, bad_dist, ctx=ctx)
    graph = (np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.array([1.0, 1.0]))
    for kw in (dict(n_components=0), dict(n_components=17), dict(n_epochs=0), dict(negative_sample_rate=-1),
               dict(init=np.zeros((3, 2))), dict(init=np.zeros(4))):
        args = dict(n_components=2, a=1.5, b=0.9, n_epochs=5, seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            engine.umap_layout(graph, ctx=ctx, **args)
    with pytest.raises(ValueError):
        engine.umap_layout((np.array([0], np.int64), graph[1], graph[2]), 2, 1.5, 0.9, 5, 1, ctx=ctx)
    with pytest.raises(ValueError):
        engine.umap_layout((graph[0], graph[1], graph[2][:1]), 2, 1.5, 0.9, 5, 1, ctx=ctx)
    assert engine.umap_default_epochs(10000) == 500 and engine.umap_default_epochs(10001) == 200


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_umap_graph", "karma_umap_layout", "karma_umap_ab", "karma_umap_tile"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_umap_graph.argtypes) == 14 and len(lib.karma_umap_layout.argtypes) == 18
    assert _lib.umap_tile() >= 64  # host only: no device needed
    assert lib.karma_umap_tile(None) == _lib.KARMA_ERR_ARG
    assert b"karma_umap_tile" in lib.karma_last_error()
    a, b = ctypes.c_double(0), ctypes.c_double(0)
    assert lib.karma_umap_ab(1.0, 0.1, None, ctypes.byref(b)) == _lib.KARMA_ERR_ARG
    assert lib.karma_umap_ab(0.0, 0.1, ctypes.byref(a), ctypes.byref(b)) == _lib.KARMA_ERR_ARG


def test_graph_argument_errors_come_before_a_device():
    lib = _lib.load()
    n, k = 6, 3
    idx = np.tile(np.arange(k, dtype=np.int32), (n, 1))
    dist = np.zeros((n, k))
    cap = 2 * n * k
    indptr, indices, weights = np.full(n + 1, -7, np.int64), np.full(cap, -7, np.int32), np.full(cap, -7.0)
    nnz = ctypes.c_int64(-7)

    def rc(ctx=None, idx=_lib.ptr(idx), dist=_lib.ptr(dist), n=n, k=k, indptr=_lib.ptr(indptr),
           indices=_lib.ptr(indices), weights=_lib.ptr(weights), cap=cap, nnz=ctypes.byref(nnz)):
        return lib.karma_umap_graph(ctx, idx, dist, n, k, 0, indptr, indices, weights, cap, nnz, None, None, 0)

    bad_idx = idx.copy()
    bad_idx[n - 1, k - 1] = n
    cases = [(dict(idx=None), b"null pointer"), (dict(dist=None), b"null pointer"),
             (dict(indptr=None), b"null pointer"), (dict(indices=None), b"null pointer"), (dict(weights=None), b"null pointer"),
             (dict(nnz=None), b"null pointer"),
             (dict(n=1), b"2 <= n < 2^31"), (dict(n=1 << 31), b"2 <= n < 2^31"),
             (dict(k=1), b"2 <= k <= min(n, 64)"), (dict(k=n + 1), b"2 <= k <= min(n, 64)"),
             (dict(n=1000, k=65), b"2 <= k <= min(n, 64)"),
             (dict(cap=cap - 1), b"2 n k entries"),
             (dict(n=1 << 25, k=64, cap=1 << 40), b"2 n k < 2^32"),
             (dict(dist=ctypes.c_void_p(dist.ctypes.data + 4)), b"8-byte aligned"),
             (dict(idx=ctypes.c_void_p(idx.ctypes.data + 2)), b"4-byte aligned"),
             (dict(idx=_lib.ptr(bad_idx)), b"neighbour index outside"),
             (dict(), b"null context")]  # every argument in order: only the context is missing
    for kw, text in cases:
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert text in lib.karma_last_error(), (kw, lib.karma_last_error())
    assert (indptr == -7).all() and (indices == -7).all() and (weights == -7.0).all() and nnz.value == -7


def test_layout_argument_errors_come_before_a_device():
    lib = _lib.load()
    n, dim = 4, 2
    indptr = np.array([0, 1, 3, 4, 4], np.int64)
    indices = np.array([1, 0, 2, 1], np.int32)
    weights = np.array([1.0, 1.0, 0.5, 0.5])
    y = np.full((n, dim), -7.0)

    def rc(ctx=None, indptr=indptr, indices=indices, weights=weights, n=n, nnz=4, dim=dim, a=1.5, b=0.9, epochs=5,
           rate=5, gamma=1.0, alpha=1.0, y=_lib.ptr(y)):
        return lib.karma_umap_layout(ctx, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(weights), n, nnz, 0, dim, a, b,
                                     epochs, rate, gamma, alpha, 1, 1, y, 0)

    def arr(base, at, value):
        out = base.copy()
        out[at] = value
        return out

    cases = [(dict(indptr=None), b"null pointer"), (dict(indices=None), b"null pointer"),
             (dict(weights=None), b"null pointer"), (dict(y=None), b"null pointer"),
             (dict(n=1), b"2 <= n < 2^31"), (dict(nnz=-1), b"nnz must not be negative"),
             (dict(dim=0), b"1 <= dim <= 16"), (dict(dim=17), b"1 <= dim <= 16"),
             (dict(epochs=0), b"n_epochs >= 1"), (dict(rate=-1), b"negative_sample_rate"),
             (dict(a=float("nan")), b"must be finite"), (dict(alpha=float("inf")), b"must be finite"),
             (dict(y=ctypes.c_void_p(y.ctypes.data + 4)), b"8-byte aligned"),
             (dict(nnz=3), b"end at nnz"), (dict(indptr=arr(indptr, 1, 4)), b"not decrease"),
             (dict(indptr=arr(indptr, 0, 1)), b"start at 0"),
             (dict(indices=arr(indices, 2, n)), b"column outside"),
             (dict(indices=arr(indices, 0, -1)), b"column outside"),
             (dict(weights=arr(weights, 3, 0.0)), b"finite and > 0"),
             (dict(weights=arr(weights, 0, float("nan"))), b"finite and > 0"),
             (dict(), b"null context")]
    for kw, text in cases:
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert text in lib.karma_last_error(), (kw, lib.karma_last_error())
    assert (y == -7.0).all()


def test_argument_checks_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "umap_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "umap_args_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_umap_headers_are_host_only():
    for name in ("umap_args.h", "umap_math.h"):
        hdr = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
