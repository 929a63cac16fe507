"""The spectral entries without a device: engine's own argument checks, the ABI's
declaration of the entries, the library's argument errors with no context, the
host eigensolver against numpy, and the checks and small dense problems
(csrc/spectral_args.h, csrc/spectral_small.h) in a stand-alone program built
with AddressSanitizer + UBSan.  The kernels themselves: tests/test_gpu_spectral.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from karma_amd import _lib, engine
from karma_amd.kmer import KmerClustering

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "karma_amd", "csrc")

INDPTR = np.array([0, 1, 3, 4, 4], np.int64)  # a path 0 - 1 - 2 and an empty row
INDICES = np.array([1, 0, 2, 1], np.int32)
WEIGHTS = np.array([1.0, 1.0, 0.5, 0.5])


class NoContext:
    """Stands where a context would: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the argument check must come before the library is reached")


def test_engine_argument_errors():
    ctx = NoContext()
    graph = (INDPTR, INDICES, WEIGHTS)
    for kw in (dict(n_components=0), dict(n_components=17), dict(tol=0.0), dict(tol=float("nan")),
               dict(tol=float("inf")), dict(max_outer=0)):
        args = dict(n_components=2, seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            engine.umap_spectral(graph, ctx=ctx, **args)
    with pytest.raises(ValueError):
        engine.umap_spectral((np.array([0, 0], np.int64), INDICES[:0], WEIGHTS[:0]), 2, 1, ctx=ctx)  # n = 1
    with pytest.raises(ValueError):
        engine.umap_spectral((INDPTR, INDICES, WEIGHTS[:3]), 2, 1, ctx=ctx)
    with pytest.raises(ValueError):
        engine.graph_components((np.array([0], np.int64), INDICES[:0]), ctx=ctx)  # n = 0
    for x in (np.zeros((3, 2)), np.zeros((4, 33)), np.zeros(4), np.zeros((4, 0))):
        with pytest.raises(ValueError):
            engine.spectral_apply(graph, x, ctx=ctx)
    with pytest.raises(ValueError, match="init must be"):
        engine.umap(np.zeros((5, 3)), init="pca", ctx=ctx)


def test_run_wants_the_device_layout_for_a_spectral_start(tmp_path):
    job = KmerClustering({">a": "ACGT"}, str(tmp_path), "5p6", 1)
    with pytest.raises(ValueError, match="device_umap=True"):
        job.run(15, 10, 0.1, 42, 5, umap_init="spectral")
    with pytest.raises(ValueError, match="umap_init must be"):
        job.run(15, 10, 0.1, 42, 5, device_umap=True, umap_init="pca")


def test_abi_declares_the_entries():
    lib = _lib.load()
    for name in ("karma_graph_components", "karma_spectral_apply", "karma_umap_spectral", "karma_spectral_tile",
                 "karma_spectral_jacobi"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert len(lib.karma_graph_components.argtypes) == 9 and len(lib.karma_spectral_apply.argtypes) == 11
    assert len(lib.karma_umap_spectral.argtypes) == 18
    tile, guard, degree = _lib.spectral_tile()  # host only: no device needed
    assert tile >= 32 and guard >= 1 and 16 + guard <= 32 and degree >= 2
    assert lib.karma_spectral_tile(None, None, None) == _lib.KARMA_ERR_ARG
    assert b"karma_spectral_tile" in lib.karma_last_error()


def _arr(base, at, value):
    out = base.copy()
    out[at] = value
    return out


def test_components_argument_errors_come_before_a_device():
    lib = _lib.load()
    comp = np.full(4, -7, np.int32)
    count = ctypes.c_int64(-7)

    def rc(ctx=None, indptr=INDPTR, indices=INDICES, n=4, nnz=4, comp=_lib.ptr(comp), count=ctypes.byref(count)):
        return lib.karma_graph_components(ctx, _lib.ptr(indptr), _lib.ptr(indices), n, nnz, 0, comp, 0, count)

    cases = [(dict(indptr=None), b"null pointer"), (dict(indices=None), b"null pointer"),
             (dict(comp=None), b"null pointer"), (dict(count=None), b"null pointer"),
             (dict(n=0), b"1 <= n"), (dict(n=1 << 31), b"n < 2^31"), (dict(nnz=-1), b"nnz must not be negative"),
             (dict(comp=ctypes.c_void_p(comp.ctypes.data + 2)), b"4-byte aligned"),
             (dict(nnz=3), b"end at nnz"), (dict(indptr=_arr(INDPTR, 1, 4)), b"not decrease"),
             (dict(indices=_arr(INDICES, 2, 4)), b"column outside"),
             (dict(indices=_arr(INDICES, 0, -1)), b"column outside"),
             (dict(), b"null context")]
    for kw, text in cases:
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert text in lib.karma_last_error(), (kw, lib.karma_last_error())
    assert (comp == -7).all() and count.value == -7


def test_apply_argument_errors_come_before_a_device():
    lib = _lib.load()
    x, out = np.ones((4, 3)), np.full((4, 3), -7.0)

    def rc(ctx=None, indptr=INDPTR, indices=INDICES, weights=WEIGHTS, n=4, nnz=4, x=_lib.ptr(x), p=3,
           out=_lib.ptr(out)):
        return lib.karma_spectral_apply(ctx, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(weights), n, nnz, 0, x, p,
                                        out, 0)

    cases = [(dict(weights=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"),
             (dict(n=1), b"2 <= n < 2^31"), (dict(p=0), b"1 <= p <= 32"), (dict(p=33), b"1 <= p <= 32"),
             (dict(out=ctypes.c_void_p(out.ctypes.data + 4)), b"8-byte aligned"),
             (dict(weights=_arr(WEIGHTS, 3, 0.0)), b"finite and > 0"),
             (dict(indices=_arr(INDICES, 2, 4)), b"column outside"),
             (dict(), b"null context")]
    for kw, text in cases:
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert text in lib.karma_last_error(), (kw, lib.karma_last_error())
    assert (out == -7.0).all()


def test_spectral_argument_errors_come_before_a_device():
    lib = _lib.load()
    n, dim = 4, 2
    y, vec, lam, res = (np.full((n, dim), -7.0) for _ in range(4))
    comp = np.full(n, -7, np.int32)
    info = np.full(4, -7, np.int64)

    def rc(ctx=None, indptr=INDPTR, indices=INDICES, weights=WEIGHTS, n=n, nnz=4, dim=dim, tol=1e-4, outer=100,
           y=_lib.ptr(y), vec=_lib.ptr(vec), info=_lib.ptr(info)):
        return lib.karma_umap_spectral(ctx, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(weights), n, nnz, 0, dim, 1,
                                       tol, outer, y, vec, _lib.ptr(lam), _lib.ptr(res), _lib.ptr(comp), 0, info)

    cases = [(dict(indptr=None), b"null pointer"), (dict(indices=None), b"null pointer"),
             (dict(weights=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(info=None), b"null pointer"),
             (dict(n=1), b"2 <= n < 2^31"), (dict(nnz=-1), b"nnz must not be negative"),
             (dict(dim=0), b"1 <= dim <= 16"), (dict(dim=17), b"1 <= dim <= 16"),
             (dict(tol=0.0), b"tol must be finite and > 0"), (dict(tol=-1.0), b"tol must be finite and > 0"),
             (dict(tol=float("nan")), b"tol must be finite and > 0"),
             (dict(tol=float("inf")), b"tol must be finite and > 0"),
             (dict(outer=0), b"max_outer >= 1"),
             (dict(y=ctypes.c_void_p(y.ctypes.data + 4)), b"8-byte aligned"),
             (dict(vec=ctypes.c_void_p(vec.ctypes.data + 4)), b"8-byte aligned"),
             (dict(nnz=3), b"end at nnz"), (dict(indptr=_arr(INDPTR, 1, 4)), b"not decrease"),
             (dict(indptr=_arr(INDPTR, 0, 1)), b"start at 0"),
             (dict(indices=_arr(INDICES, 2, n)), b"column outside"),
             (dict(weights=_arr(WEIGHTS, 3, 0.0)), b"finite and > 0"),
             (dict(weights=_arr(WEIGHTS, 0, float("nan"))), b"finite and > 0"),
             (dict(), b"null context")]
    for kw, text in cases:
        assert rc(**kw) == _lib.KARMA_ERR_ARG, kw
        assert text in lib.karma_last_error(), (kw, lib.karma_last_error())
    for out in (y, vec, lam, res):
        assert (out == -7.0).all()
    assert (comp == -7).all() and (info == -7).all()


def _jacobi(a):
    lib = _lib.load()
    p = len(a)
    a = np.ascontiguousarray(a, np.float64)
    w, v = np.empty(p), np.empty((p, p))
    assert lib.karma_spectral_jacobi(_lib.ptr(a), p, _lib.ptr(w), _lib.ptr(v)) == _lib.KARMA_OK
    return w, v


def _check_jacobi(a):
    p = len(a)
    w, v = _jacobi(a)
    want = np.linalg.eigvalsh(a)[::-1]
    scale = max(np.abs(want).max(), 1e-300)
    assert np.abs(w - want).max() <= 1e-12 * scale
    assert np.abs(v.T @ v - np.eye(p)).max() <= 1e-12
    assert np.abs(a @ v - v * w).max() <= 1e-12 * scale  # every column an eigenvector, degenerate ones included
    assert (np.diff(w) <= 0).all()


@pytest.mark.parametrize("p", [1, 2, 17, 32])
def test_jacobi_equals_eigh(p):
    rng = np.random.default_rng(900 + p)
    a = rng.normal(size=(p, p))
    _check_jacobi(a + a.T)
    _check_jacobi((a + a.T) * 1e-9)  # the threshold is relative to the matrix


def test_jacobi_on_a_rank_deficient_gram_and_on_repeated_eigenvalues():
    rng = np.random.default_rng(910)
    b = rng.normal(size=(5, 17))  # 17 vectors in 5 dimensions: 12 null directions
    _check_jacobi(b.T @ b)
    w, _ = _jacobi(b.T @ b)
    assert np.abs(w[5:]).max() <= 1e-12 * w[0] and w[4] > 1e-3 * w[0]
    q, _ = np.linalg.qr(rng.normal(size=(17, 17)))
    d = np.repeat([3.0, 1.0, -2.0], [5, 7, 5])
    _check_jacobi(q @ np.diag(d) @ q.T)
    _check_jacobi(np.eye(32))
    _check_jacobi(np.zeros((4, 4)))


def test_jacobi_rejects_bad_arguments():
    lib = _lib.load()
    a, w, v = np.eye(2), np.empty(2), np.empty((2, 2))
    assert lib.karma_spectral_jacobi(None, 2, _lib.ptr(w), _lib.ptr(v)) == _lib.KARMA_ERR_ARG
    assert lib.karma_spectral_jacobi(_lib.ptr(a), 0, _lib.ptr(w), _lib.ptr(v)) == _lib.KARMA_ERR_ARG
    assert lib.karma_spectral_jacobi(_lib.ptr(a), 34, _lib.ptr(w), _lib.ptr(v)) == _lib.KARMA_ERR_ARG


def test_argument_checks_under_sanitizers():
    subprocess.run(["make", "-C", CSRC, "spectral_args_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "build", "spectral_args_test")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok (")


def test_spectral_headers_are_host_only():
    for name in ("spectral_args.h", "spectral_small.h"):
        hdr = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in hdr and "karma_internal.h\"" not in hdr
