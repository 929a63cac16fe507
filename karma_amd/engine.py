"""Host-side driver of the HIP hot path (thin layer over karma_amd._lib).

Everything here moves host arrays to/from libkarma_hip.so; all compute is in
the HIP kernels (karma_amd/csrc/*.hip).  The drop-in classes (kmer.py,
read_graph.py, contig.py) call these functions.
"""

from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import call, ptr
from .logs import logger

KMODE_5P6 = _lib.KARMA_KMER_5P6


def kmode_of(kmer_size) -> int:
    """kmer.py:69 tests `kmer_size == "5p6"`; anything else is an int k
    (cmd_parser.py:234-235 casts with int())."""
    if kmer_size == "5p6":
        return KMODE_5P6
    return int(kmer_size)


def encode_sequences(sequences):
    """OrderedDict[str, str] -> (bytes blob, offsets int64[N+1], key_len int32[N]).

    Sequences are compared/sliced as Python str; for code points < 256 latin-1
    bytes preserve both length and ordering, so the byte kernels are exact.
    """
    vals = []
    for v in sequences.values():
        try:
            vals.append(v.encode("latin-1"))
        except UnicodeEncodeError as e:
            raise ValueError("sequence contains a code point >= 256; libkarma_hip handles byte sequences "
                             "(latin-1) only") from e
    offs = np.zeros(len(vals) + 1, dtype=np.int64)
    if vals:
        np.cumsum([len(v) for v in vals], out=offs[1:])
    blob = np.frombuffer(b"".join(vals) + b"\0" * 16, dtype=np.uint8)
    key_len = np.array([len(k) for k in sequences.keys()], dtype=np.int32)
    return blob, offs, key_len


def decode_keys(keys: np.ndarray, kmode: int):
    """u64 column keys (karma.h encoding) -> list[str] (latin-1)."""
    out = []
    for k in keys.tolist():
        if kmode == 8:
            ln = 8
        else:
            ln = k & 0xFF
        b = k.to_bytes(8, "big")[:ln]
        out.append(b.decode("latin-1"))
    return out


class ContigStore:
    """Device-resident contigs (karma_contigs): 2-bit packed + exception mask."""

    def __init__(self, ctx, blob, offsets, key_len, device_pointers=False, n=None):
        self.ctx = ctx
        h = ctypes.c_void_p()
        if device_pointers:
            call("karma_contigs_create", ctx.h, ctypes.c_void_p(blob), ctypes.c_void_p(offsets),
                 ctypes.c_void_p(key_len), n, 1, ctypes.byref(h))
        else:
            self._keep = (blob, offsets, key_len)
            n = len(key_len)
            call("karma_contigs_create", ctx.h, ptr(blob), ptr(offsets), ptr(key_len) if n else ptr(
                np.zeros(1, np.int32)), n, 0, ctypes.byref(h))
        self.h = h
        self.n = n

    def info(self):
        v = [ctypes.c_int64() for _ in range(4)]
        call("karma_contigs_info", self.h, *[ctypes.byref(x) for x in v])
        return dict(n=v[0].value, total_bases=v[1].value, exception_bases=v[2].value, packed_bytes=v[3].value)

    def words(self):
        """The packed store on the host (karma_contigs_words): (packed uint32[W], mask uint16[W],
        word offsets int64[n + 1], exception flag uint8[n])."""
        woff = np.zeros(self.n + 1, np.int64)
        call("karma_contigs_words", self.h, None, None, ptr(woff), None)
        W = int(woff[-1])
        packed, mask, has_exc = np.zeros(W, np.uint32), np.zeros(W, np.uint16), np.zeros(self.n, np.uint8)
        call("karma_contigs_words", self.h, ptr(packed) if W else None, ptr(mask) if W else None, None,
             ptr(has_exc) if self.n else None)
        return packed, mask, woff, has_exc

    def close(self):
        if getattr(self, "h", None):
            _lib.load().karma_contigs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class KmerPlan:
    """Presence pass + column table + dense profile (karma_kmer_plan)."""

    def __init__(self, ctx, store: ContigStore, kmode: int):
        self.ctx, self.store, self.kmode = ctx, store, kmode
        h = ctypes.c_void_p()
        call("karma_kmer_plan_create", ctx.h, store.h, kmode, ctypes.byref(h))
        self.h = h
        self.M = None

    # -- exchange points (multi-rank) --
    def presence_words(self):
        n = ctypes.c_int64()
        call("karma_kmer_presence_words", self.h, ctypes.byref(n))
        return n.value

    def presence_get(self, dst_dev_ptr):
        call("karma_kmer_presence_get", self.h, ctypes.c_void_p(dst_dev_ptr))

    def presence_set(self, src_dev_ptr):
        call("karma_kmer_presence_set", self.h, ctypes.c_void_p(src_dev_ptr))

    def presence_merge(self, all_dev_ptr, n_sets):
        """Presence = OR of n_sets bitmaps back to back in device memory."""
        call("karma_kmer_presence_merge", self.h, ctypes.c_void_p(all_dev_ptr), int(n_sets))

    def exceptions_count(self):
        n = ctypes.c_int64()
        call("karma_kmer_exceptions_count", self.h, ctypes.byref(n))
        return n.value

    def exceptions_get(self, dst_dev_ptr):
        call("karma_kmer_exceptions_get", self.h, ctypes.c_void_p(dst_dev_ptr) if dst_dev_ptr else None)

    def exceptions_set(self, src_dev_ptr, n):
        call("karma_kmer_exceptions_set", self.h, ctypes.c_void_p(src_dev_ptr) if src_dev_ptr else None, n)

    def finalize(self):
        m = ctypes.c_int64()
        call("karma_kmer_plan_finalize", self.h, ctypes.byref(m))
        self.M = m.value
        return self.M

    def finalize_async(self):
        """Enqueue the column table; finalize_wait() returns M."""
        call("karma_kmer_plan_finalize_async", self.h)

    def finalize_wait(self):
        m = ctypes.c_int64()
        call("karma_kmer_plan_finalize_wait", self.h, ctypes.byref(m))
        self.M = m.value
        return self.M

    def columns(self):
        keys = np.zeros(max(self.M, 1), dtype=np.uint64)
        call("karma_kmer_columns", self.h, ptr(keys))
        return keys[: self.M]

    def profile_path(self, use_cap=False):
        """The kernel the profile runs (karma_kmer_profile_path): 0 wave u16, 1 wave u32, 2 block with LDS
        counts, 3 block with scratch rows; use_cap: chosen on the column capacity, as the deferred step does."""
        v = ctypes.c_int(-1)
        call("karma_kmer_profile_path", self.h, 1 if use_cap else 0, ctypes.byref(v))
        return v.value

    def row_totals(self):
        out = np.zeros(max(self.store.n, 1), dtype=np.int64)
        call("karma_kmer_row_totals", self.h, ptr(out))
        return out[: self.store.n]

    def profile_host(self):
        out = np.zeros((self.store.n, self.M), dtype=np.float64)
        if out.size:
            call("karma_kmer_profile", self.h, ptr(out), self.M, 0)
        return out

    def profile_rows(self, lo, hi, out):
        """Rows [lo, hi) into a host float64 array of hi - lo rows (C order,
        row stride = its second dimension >= M)."""
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape[0] == hi - lo
        if hi > lo:
            call("karma_kmer_profile_rows", self.h, lo, hi, ptr(out), out.shape[1], 0)

    def profile_device(self, dst_dev_ptr, ld=None):
        call("karma_kmer_profile", self.h, ctypes.c_void_p(dst_dev_ptr), ld or self.M, 1)

    def profile_side(self, dst_dev_ptr, side_stream_ptr, ld=None):
        """profile_device on a side stream, after the work already enqueued on the
        context's stream; the context joins it with Context.join(side)."""
        call("karma_kmer_profile_side", self.h, ctypes.c_void_p(dst_dev_ptr), ld or self.M,
             ctypes.c_void_p(side_stream_ptr))

    def close(self):
        if getattr(self, "h", None):
            _lib.load().karma_kmer_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


BLOCK_BYTES = 4 << 30  # row blocks of a streamed profile (device buffer and D2H unit)


def kmer_profile(sequences, kmer_size, ctx=None, out=None, block_bytes=None):
    """Full single-device k-mer profile of an OrderedDict (kmer.py:199-233).

    out: None (a new array), or a caller float64[N, M] C-order array -- a
    numpy.memmap for a profile larger than host memory -- that is filled one
    row block (~block_bytes) at a time (SURVEY.md §8(e) streaming).  Its shape
    must be (N, M); M is the column count the sequences give (kmer_columns).
    Returns (profile, columns list[str], row_totals int64[N])."""
    ctx = ctx or _lib.default_context()
    kmode = kmode_of(kmer_size)
    packed = getattr(sequences, "karma_packed", None)  # fasta.FastaDict straight from the C++ reader
    blob, offs, key_len = packed if packed is not None else encode_sequences(sequences)
    store = ContigStore(ctx, blob, offs, key_len)
    try:
        plan = KmerPlan(ctx, store, kmode)
        try:
            M = plan.finalize()
            cols = decode_keys(plan.columns(), kmode)
            n = store.n
            big = n * M * 8 > (block_bytes or BLOCK_BYTES)
            if out is None and not big:
                prof = plan.profile_host()
            else:
                if out is None:
                    out = np.empty((n, M), np.float64)
                if out.shape != (n, M) or out.dtype != np.float64 or not out.flags.c_contiguous:
                    raise ValueError(f"out must be a C-order float64 array of shape {(n, M)}")
                for lo, hi, blk in _row_blocks(plan, n, M, block_bytes):
                    out[lo:hi] = blk
                prof = out
            tot = plan.row_totals()
        finally:
            plan.close()
    finally:
        store.close()
    return prof, cols, tot


def _row_blocks(plan, n, M, block_bytes=None, ring=1):
    """(lo, hi, block) over the profile's rows; blocks are host arrays reused
    round-robin from a ring of `ring` (a consumer may hold ring - 1 of them)."""
    rows = max(1, min(n, (block_bytes or BLOCK_BYTES) // max(1, 8 * M)))
    bufs = [np.empty((rows, M), np.float64) for _ in range(max(1, ring))]
    for i, lo in enumerate(range(0, n, rows)):
        hi = min(n, lo + rows)
        blk = bufs[i % len(bufs)][: hi - lo]
        plan.profile_rows(lo, hi, blk)  # M == 0: the row totals only
        yield lo, hi, blk


def kmer_profile_blocks(sequences, kmer_size, block_rows, ctx=None, ring=1):
    """The profile as a stream of (lo, hi, rows float64[hi - lo, M]) row blocks
    and the column list: (columns, generator).  Block arrays are reused from a
    ring of `ring` buffers: a consumer may keep the last ring - 1 blocks while
    it advances (e.g. hash them on a thread pool).  Nothing of size N x M
    exists on the host or the device at once (SURVEY.md §8(e) C5 streaming)."""
    ctx = ctx or _lib.default_context()
    kmode = kmode_of(kmer_size)
    packed = getattr(sequences, "karma_packed", None)
    blob, offs, key_len = packed if packed is not None else encode_sequences(sequences)
    store = ContigStore(ctx, blob, offs, key_len)
    plan = KmerPlan(ctx, store, kmode)
    M = plan.finalize()
    cols = decode_keys(plan.columns(), kmode)

    def gen():
        try:
            yield from _row_blocks(plan, store.n, M, block_rows * max(1, 8 * M), ring)
        finally:
            plan.close()
            store.close()

    return cols, gen()


def kmer_columns_count(sequences, kmer_size, ctx=None):
    """M: the number of columns (present k-mers) of the sequences' profile."""
    ctx = ctx or _lib.default_context()
    kmode = kmode_of(kmer_size)
    packed = getattr(sequences, "karma_packed", None)
    blob, offs, key_len = packed if packed is not None else encode_sequences(sequences)
    store = ContigStore(ctx, blob, offs, key_len)
    try:
        plan = KmerPlan(ctx, store, kmode)
        try:
            return plan.finalize()
        finally:
            plan.close()
    finally:
        store.close()


def kmer_profile_device(sequences, kmer_size, ctx=None):
    """kmer_profile with the profile left in HBM:
    returns (DeviceProfile, columns list[str], row_totals int64[N]); nothing of
    size N x M crosses PCIe."""
    from .device_profile import profile_to_device

    ctx = ctx or _lib.default_context()
    kmode = kmode_of(kmer_size)
    packed = getattr(sequences, "karma_packed", None)
    blob, offs, key_len = packed if packed is not None else encode_sequences(sequences)
    store = ContigStore(ctx, blob, offs, key_len)
    try:
        plan = KmerPlan(ctx, store, kmode)
        try:
            plan.finalize()
            cols = decode_keys(plan.columns(), kmode)
            dev = profile_to_device(ctx, plan, cols)
            tot = plan.row_totals()
        finally:
            plan.close()
    finally:
        store.close()
    return dev, cols, tot


def _knn_source(x):
    """(host array or None, device pointer or None, n, M, ld) of a matrix knn_rows accepts."""
    from .device_profile import DeviceProfile

    if isinstance(x, DeviceProfile):
        if x._buf is None:
            raise ValueError("DeviceProfile is closed")
        n, M = x.shape
        return None, x.ptr, n, M, M
    if isinstance(x, _lib.DevBuf):
        if len(x.shape) != 2 or x.dtype != np.float64:
            raise ValueError(f"a device matrix must be float64 (n, M), not {x.dtype} {x.shape}")
        if x.ptr is None:
            raise ValueError("DevBuf is closed")
        n, M = x.shape
        return None, x.ptr, n, M, M
    a = np.asarray(x)
    if a.dtype != np.float64:
        raise TypeError(f"the matrix must be float64 (distances are defined on its bits), not {a.dtype}")
    if a.ndim != 2:
        raise ValueError(f"the matrix must have shape (n, M), not {a.shape}")
    n, M = a.shape
    # rows of a wider C-order array keep their stride (ld); anything else is copied compact
    if not (n and M and a.strides[1] == 8 and a.strides[0] >= 8 * M and a.strides[0] % 8 == 0):
        a = np.ascontiguousarray(a)
    return a, None, n, M, (a.strides[0] // 8 if n and M else M)


def knn_rows(x, k, row_lo=0, row_hi=None, ctx=None, out_device=False):
    """Exact k nearest rows of the float64 matrix x (n, M) for the query rows
    [row_lo, row_hi) (karma_knn_rows; the contract is in include/karma.h):
    d2 accumulated column by column as acc + t * t, the k smallest (d2, index)
    among all n rows, the row itself included.  x: a numpy array, a DevBuf or a
    DeviceProfile.  Returns (idx int32[rows, k], dist float64[rows, k]): numpy
    arrays, or DevBufs with out_device=True.  1 <= k <= min(n, 64); an empty
    range gives empty arrays."""
    host, dptr, n, M, ld = _knn_source(x)
    k = int(k)
    row_lo = int(row_lo)
    row_hi = n if row_hi is None else int(row_hi)
    if not 0 <= row_lo <= row_hi <= n:
        raise ValueError(f"need 0 <= row_lo <= row_hi <= n, not [{row_lo}, {row_hi}) of {n} rows")
    k_max = _lib.knn_tile()[3]
    if k < 1 or (row_hi > row_lo and k > min(n, k_max)):
        raise ValueError(f"need 1 <= k <= min(n, {k_max}), not k = {k} with n = {n}")
    rows = row_hi - row_lo
    if ctx is None:
        ctx = x.ctx if host is None else _lib.default_context()
    if out_device:
        idx, dist = _lib.DevBuf(ctx, (rows, k), np.int32), _lib.DevBuf(ctx, (rows, k), np.float64)
        pi, pd = ctypes.c_void_p(idx.ptr), ctypes.c_void_p(dist.ptr)
    else:
        idx, dist = np.empty((rows, k), np.int32), np.empty((rows, k), np.float64)
        pi, pd = ptr(idx), ptr(dist)
    if rows:
        src = ctypes.c_void_p(dptr) if host is None else ptr(host)
        call("karma_knn_rows", ctx.h, src, n, M, ld, 1 if host is None else 0, row_lo, row_hi, k, pi, pd,
             1 if out_device else 0)
    return idx, dist


def _mst_min_samples(min_samples, n):
    min_samples = int(min_samples)
    k_max = _lib.knn_tile()[3]
    if n < 1:
        raise ValueError("the matrix must have at least one row")
    if min_samples < 1 or min_samples > min(n, k_max):
        raise ValueError(f"need 1 <= min_samples <= min(n, {k_max}), not min_samples = {min_samples} with n = {n}")
    return min_samples


def mreach_mst(x, min_samples, ctx=None):
    """The exact minimum spanning tree of the mutual-reachability graph of the
    rows of the float64 matrix x (n, M) (karma_mreach_mst; the contract is in
    include/karma.h): d2 as knn_rows defines it, core2(i) the min_samples-th
    smallest (d2(i, j), j) with row i counted, mr2 = max(d2, core2(i),
    core2(j)), and the one tree under the order (mr2, lo, hi).  x: what
    knn_rows accepts.  Returns (a int32[n-1], b int32[n-1], w float64[n-1],
    core float64[n]): the edges ascending by that key, a < b, w = sqrt(mr2),
    core = sqrt(core2)."""
    host, dptr, n, M, ld = _knn_source(x)
    min_samples = _mst_min_samples(min_samples, n)
    if ctx is None:
        ctx = x.ctx if host is None else _lib.default_context()
    a, b = np.empty(n - 1, np.int32), np.empty(n - 1, np.int32)
    w, core = np.empty(n - 1, np.float64), np.empty(n, np.float64)
    src = ctypes.c_void_p(dptr) if host is None else ptr(host)
    call("karma_mreach_mst", ctx.h, src, n, M, ld, 1 if host is None else 0, min_samples, ptr(a), ptr(b), ptr(w),
         ptr(core), 0)
    return a, b, w, core


def _min_cluster_size(min_cluster_size):
    min_cluster_size = int(min_cluster_size)
    if min_cluster_size < 2:
        raise ValueError(f"need min_cluster_size >= 2, not {min_cluster_size}")
    return min_cluster_size


def hdbscan_tree(a, b, w, n, min_cluster_size, allow_single_cluster=False):
    """HDBSCAN's labels from a spanning tree's edges, on the host
    (karma_hdbscan_tree; include/karma.h): single linkage of the n - 1 edges in
    the order given (w must not decrease), the condensed tree, excess of mass,
    labels.  Returns (labels int32[n], probabilities float64[n]); noise is -1."""
    n = int(n)
    min_cluster_size = _min_cluster_size(min_cluster_size)
    if n < 1:
        raise ValueError("need n >= 1")
    a = np.ascontiguousarray(a, np.int32)
    b = np.ascontiguousarray(b, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    if not a.shape == b.shape == w.shape == (n - 1,):
        raise ValueError(f"a, b and w must each hold n - 1 = {n - 1} edges, not {a.shape}, {b.shape}, {w.shape}")
    labels, prob = np.empty(n, np.int32), np.empty(n, np.float64)
    count = ctypes.c_int32(0)
    call("karma_hdbscan_tree", n, ptr(a), ptr(b), ptr(w), min_cluster_size, 1 if allow_single_cluster else 0,
         ptr(labels), ptr(prob), ctypes.byref(count))
    return labels, prob


class HdbscanResult:
    """What engine.hdbscan returns: labels_ (int32, noise -1) and
    probabilities_ (float64), as a fitted clusterer's attributes are named."""

    def __init__(self, labels, probabilities):
        self.labels_ = labels
        self.probabilities_ = probabilities


def hdbscan(x, min_cluster_size=5, min_samples=None, allow_single_cluster=False, ctx=None):
    """HDBSCAN of the rows of the float64 matrix x (n, M): the exact
    mutual-reachability spanning tree on the device (mreach_mst) and the
    cluster tree on the host (hdbscan_tree).  min_samples=None means
    min_cluster_size; a point counts among its own neighbours, as in
    scikit-learn.  Every bit of the result is defined by include/karma.h; it is
    not claimed to equal the `hdbscan` package's labels (its default tree is
    approximate and its tie order its own)."""
    min_cluster_size = _min_cluster_size(min_cluster_size)
    host, _, n, _, _ = _knn_source(x)
    min_samples = _mst_min_samples(min_cluster_size if min_samples is None else min_samples, n)
    a, b, w, _ = mreach_mst(x, min_samples, ctx=ctx)
    return HdbscanResult(*hdbscan_tree(a, b, w, n, min_cluster_size, allow_single_cluster))


def _on_device(*arrays):
    return all(isinstance(a, _lib.DevBuf) for a in arrays)


def _dev_or_host(a, dtype):
    """(argument for the library, the object that keeps it alive)."""
    if isinstance(a, _lib.DevBuf):
        if a.dtype != np.dtype(dtype):
            raise TypeError(f"a device array of {a.dtype} where {np.dtype(dtype)} is needed")
        if a.ptr is None:
            raise ValueError("DevBuf is closed")
        return ctypes.c_void_p(a.ptr), a
    h = np.ascontiguousarray(a, dtype=dtype)
    return ptr(h), h


def umap_graph(idx, dist, ctx=None, out_device=False, with_sigma=False):
    """UMAP's fuzzy simplicial set of exact neighbour lists (karma_umap_graph;
    the contract is in include/karma.h): idx int32[n, k] and dist float64[n, k]
    as knn_rows gives them, both numpy arrays or both DevBufs.  Returns the
    symmetric graph in CSR, (indptr int64[n+1], indices int32[nnz], weights
    float64[nnz]), each row ascending by column: numpy arrays, or DevBufs with
    out_device=True.  with_sigma=True appends (sigma, rho), float64[n] each.
    2 <= k <= min(n, 64)."""
    device = _on_device(idx, dist)
    if not device and (isinstance(idx, _lib.DevBuf) or isinstance(dist, _lib.DevBuf)):
        raise TypeError("idx and dist must both be numpy arrays or both be DevBufs")
    shape = tuple(idx.shape) if device else np.shape(idx)
    if len(shape) != 2 or tuple(dist.shape if device else np.shape(dist)) != shape:
        raise ValueError("idx and dist must have the same shape (n, k)")
    n, k = shape
    k_max = _lib.knn_tile()[3]
    if n < 2 or k < 2 or k > min(n, k_max):
        raise ValueError(f"need n >= 2 and 2 <= k <= min(n, {k_max}), not n = {n}, k = {k}")
    if ctx is None:
        ctx = idx.ctx if device else _lib.default_context()
    pi, keep_i = _dev_or_host(idx, np.int32)
    pd, keep_d = _dev_or_host(dist, np.float64)
    cap = 2 * n * k
    nnz = ctypes.c_int64(0)

    def make(count, dtype):
        return _lib.DevBuf(ctx, (count,), dtype) if out_device else np.empty(count, dtype)

    def arg(buf):
        return ctypes.c_void_p(buf.ptr) if out_device else ptr(buf)

    indptr, indices, weights = make(n + 1, np.int64), make(cap, np.int32), make(cap, np.float64)
    sigma, rho = (make(n, np.float64), make(n, np.float64)) if with_sigma else (None, None)
    call("karma_umap_graph", ctx.h, pi, pd, n, k, 1 if device else 0, arg(indptr), arg(indices), arg(weights), cap,
         ctypes.byref(nnz), arg(sigma) if with_sigma else None, arg(rho) if with_sigma else None,
         1 if out_device else 0)
    if out_device:
        indices, weights = indices.view(0, nnz.value), weights.view(0, nnz.value)
    else:
        indices, weights = indices[:nnz.value].copy(), weights[:nnz.value].copy()
    return (indptr, indices, weights, sigma, rho) if with_sigma else (indptr, indices, weights)


def _mcl_options(inflation, resource, cutoff, eps, max_iter, general, cand_cap):
    inflation, resource, cutoff, eps = float(inflation), int(resource), float(cutoff), float(eps)
    max_iter, cand_cap = int(max_iter), int(cand_cap)
    if not 2 <= resource <= 32:
        raise ValueError(f"need 2 <= resource <= 32, not {resource}")
    if not 1.0 < inflation <= 16.0:
        raise ValueError(f"need 1 < inflation <= 16, not {inflation}")
    if not 2.0 ** -40 <= cutoff <= 0.5:
        raise ValueError(f"need 2^-40 <= cutoff <= 0.5, not {cutoff}")
    if not eps >= 0.0:
        raise ValueError(f"need eps >= 0, not {eps}")
    if max_iter < 1:
        raise ValueError(f"need max_iter >= 1, not {max_iter}")
    if not 0 <= cand_cap < 2 ** 32:
        raise ValueError(f"need 0 <= cand_cap < 2^32, not {cand_cap}")
    return inflation, resource, cutoff, eps, max_iter, _lib.KARMA_MCL_GENERAL if general else 0, cand_cap


def _mcl_outputs(ctx, n, resource, out_device):
    cap = n * resource

    def make(count, dtype):
        return _lib.DevBuf(ctx, (count,), dtype) if out_device else np.empty(count, dtype)

    def arg(buf):
        return ctypes.c_void_p(buf.ptr) if out_device else ptr(buf)

    return cap, make(n + 1, np.int64), make(cap, np.uint32), make(cap, np.float64), arg


def _mcl_result(ctx, n, colptr, rows, vals, out_device):
    """Trim rows and vals to the matrix's entries (a device result's count is read back)."""
    if out_device:
        last = np.zeros(1, np.int64)
        call("karma_memcpy", ctx.h, ptr(last), ctypes.c_void_p(colptr.ptr + 8 * n), 8, 1)
        return rows.view(0, int(last[0])), vals.view(0, int(last[0]))
    return rows[:colptr[n]].copy(), vals[:colptr[n]].copy()


def mcl(off, nbr, w, inflation=2.0, resource=4, cutoff=1 / 4000, eps=1e-3, max_iter=100, general=False, cand_cap=0,
        ctx=None, out_device=False):
    """Markov clustering of a weighted graph on the device (karma_mcl; the
    contract is in include/karma.h): the graph as CSR in karma_adj_get's layout,
    off int64[n + 1], nbr uint32[nnz], w float64[nnz], all numpy arrays or all
    DevBufs.  Returns (colptr int64[n + 1], rows uint32, vals float64,
    iterations, chaos): the final matrix as CSC, numpy arrays, or DevBufs with
    out_device=True.  general=True keeps every iteration on the sort-based
    general path; cand_cap bounds a batch of it (0: the default).  Every bit is
    defined by the contract; equality with the `mcl` binary's clusters is not
    claimed (its pruning is richer and has a tie order of its own)."""
    device = _on_device(off, nbr, w)
    if not device and any(isinstance(a, _lib.DevBuf) for a in (off, nbr, w)):
        raise TypeError("off, nbr and w must all be numpy arrays or all be DevBufs")
    n = int((off.shape if device else np.shape(off))[0]) - 1
    if n < 1:
        raise ValueError("need n >= 1")
    opts = _mcl_options(inflation, resource, cutoff, eps, max_iter, general, cand_cap)
    if ctx is None:
        ctx = off.ctx if device else _lib.default_context()
    po, keep_o = _dev_or_host(off, np.int64)
    pn, keep_n = _dev_or_host(nbr, np.uint32)
    pw, keep_w = _dev_or_host(w, np.float64)
    if not device and not len(keep_n) == len(keep_w) >= int(keep_o[-1]):
        raise ValueError("nbr and w must each hold off[n] entries")
    cap, colptr, rows, vals, arg = _mcl_outputs(ctx, n, opts[1], out_device)
    it, chaos = ctypes.c_int32(0), ctypes.c_double(0.0)
    call("karma_mcl", ctx.h, n, po, pn, pw, 1 if device else 0, opts[0], opts[1], opts[2], opts[3], opts[4], opts[5],
         opts[6], arg(colptr), arg(rows), arg(vals), cap, ctypes.byref(it), ctypes.byref(chaos),
         1 if out_device else 0)
    rows, vals = _mcl_result(ctx, n, colptr, rows, vals, out_device)
    return colptr, rows, vals, it.value, chaos.value


def mcl_clusters(colptr, rows, vals):
    """The clusters of a final MCL matrix, on the host (karma_mcl_clusters; no
    device needed): attractors, their systems, every node with the system that
    holds the largest mass of its column.  Returns (labels int32[n],
    n_clusters); labels rank the clusters by (size descending, smallest member
    ascending)."""
    colptr = np.ascontiguousarray(colptr, np.int64)
    rows = np.ascontiguousarray(rows, np.uint32)
    vals = np.ascontiguousarray(vals, np.float64)
    n = len(colptr) - 1
    if n < 1:
        raise ValueError("need n >= 1")
    if not len(rows) == len(vals) >= int(colptr[-1]):
        raise ValueError("rows and vals must each hold colptr[n] entries")
    labels = np.empty(n, np.int32)
    count = ctypes.c_int32(0)
    call("karma_mcl_clusters", n, ptr(colptr), ptr(rows), ptr(vals), ptr(labels), ctypes.byref(count))
    return labels, count.value


def umap_ab(spread=1.0, min_dist=0.1):
    """umap's find_ab_params (karma_umap_ab, on the host: no device needed):
    (a, b) of the curve 1 / (1 + a x^(2b)) fitted to the membership curve of
    (spread, min_dist)."""
    spread, min_dist = float(spread), float(min_dist)
    if not (np.isfinite(spread) and spread > 0 and np.isfinite(min_dist) and min_dist >= 0):
        raise ValueError(f"need spread > 0 and min_dist >= 0, not {spread}, {min_dist}")
    a, b = ctypes.c_double(0), ctypes.c_double(0)
    call("karma_umap_ab", spread, min_dist, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def umap_layout(graph, n_components, a, b, n_epochs, seed, init=None, negative_sample_rate=5, gamma=1.0,
                initial_alpha=1.0, ctx=None):
    """The layout of a symmetric CSR graph in gather form (karma_umap_layout;
    include/karma.h defines every bit): graph = (indptr, indices, weights) as
    umap_graph returns them, numpy arrays or DevBufs.  init=None starts from
    the library's uniform [-10, 10) coordinates of `seed`; a float64 (n,
    n_components) numpy array starts from it (and is not changed); a DevBuf of
    that shape is updated in place and returned.  Returns float64[n,
    n_components]."""
    indptr, indices, weights = graph[:3]
    device = _on_device(indptr, indices, weights)
    if not device and any(isinstance(x, _lib.DevBuf) for x in (indptr, indices, weights)):
        raise TypeError("the graph's three arrays must all be numpy arrays or all be DevBufs")
    dim, n_epochs, rate, seed = int(n_components), int(n_epochs), int(negative_sample_rate), int(seed)
    n = (indptr.size if device else len(indptr)) - 1
    nnz = indices.size if device else len(indices)
    if n < 2:
        raise ValueError(f"need n >= 2, not {n}")
    if not 1 <= dim <= 16:
        raise ValueError(f"need 1 <= n_components <= 16, not {dim}")
    if n_epochs < 1 or rate < 0:
        raise ValueError(f"need n_epochs >= 1 and negative_sample_rate >= 0, not {n_epochs}, {rate}")
    if (weights.size if device else len(weights)) != nnz:
        raise ValueError("indices and weights must have the same length")
    if ctx is None:
        ctx = indptr.ctx if device else _lib.default_context()
    pp, keep_p = _dev_or_host(indptr, np.int64)
    pi, keep_i = _dev_or_host(indices, np.int32)
    pw, keep_w = _dev_or_host(weights, np.float64)
    if isinstance(init, _lib.DevBuf):
        if init.dtype != np.float64 or init.shape != (n, dim):
            raise ValueError(f"init must be float64 ({n}, {dim}), not {init.dtype} {init.shape}")
        y, py, y_dev = init, ctypes.c_void_p(init.ptr), 1
    elif init is None:
        y = np.empty((n, dim), np.float64)
        py, y_dev = ptr(y), 0
    else:
        y = np.array(init, dtype=np.float64, order="C")  # a copy: the caller's start is kept
        if y.shape != (n, dim):
            raise ValueError(f"init must have shape ({n}, {dim}), not {y.shape}")
        py, y_dev = ptr(y), 0
    call("karma_umap_layout", ctx.h, pp, pi, pw, n, nnz, 1 if device else 0, dim, float(a), float(b), n_epochs, rate,
         float(gamma), float(initial_alpha), ctypes.c_uint64(seed & (2**64 - 1)), 1 if init is None else 0, py,
         y_dev)
    return y


def umap_default_epochs(n):
    """umap's rule: 500 epochs up to 10000 points, 200 above."""
    return 500 if n <= 10000 else 200


def _csr_graph(graph, need_weights=True):
    """(device, n, nnz, the three arrays) of a CSR graph given as numpy arrays or as DevBufs."""
    indptr, indices = graph[0], graph[1]
    weights = graph[2] if need_weights else None
    parts = (indptr, indices, weights) if need_weights else (indptr, indices)
    device = _on_device(*parts)
    if not device and any(isinstance(x, _lib.DevBuf) for x in parts):
        raise TypeError("the graph's arrays must all be numpy arrays or all be DevBufs")
    n = (indptr.size if device else len(indptr)) - 1
    nnz = indices.size if device else len(indices)
    if need_weights and (weights.size if device else len(weights)) != nnz:
        raise ValueError("indices and weights must have the same length")
    return device, n, nnz, indptr, indices, weights


def graph_components(graph, ctx=None, out_device=False):
    """The connected components of a CSR graph read as undirected
    (karma_graph_components): graph = (indptr, indices[, weights]), numpy
    arrays or DevBufs; the weights are not looked at.  Returns (comp, n_comp):
    comp int32[n], every vertex's smallest component member (a numpy array, or
    a DevBuf with out_device=True)."""
    device, n, nnz, indptr, indices, _ = _csr_graph(graph, need_weights=False)
    if n < 1:
        raise ValueError(f"need n >= 1, not {n}")
    if ctx is None:
        ctx = indptr.ctx if device else _lib.default_context()
    pp, keep_p = _dev_or_host(indptr, np.int64)
    pi, keep_i = _dev_or_host(indices, np.int32)
    comp = _lib.DevBuf(ctx, (n,), np.int32) if out_device else np.empty(n, np.int32)
    count = ctypes.c_int64(0)
    call("karma_graph_components", ctx.h, pp, pi, n, nnz, 1 if device else 0,
         ctypes.c_void_p(comp.ptr) if out_device else ptr(comp), 1 if out_device else 0, ctypes.byref(count))
    return comp, count.value


def spectral_apply(graph, x, ctx=None):
    """S x for the block x (float64 (n, p), p <= 32, a numpy array) and the
    normalised operator S = D^-1/2 W D^-1/2 of the CSR graph
    (karma_spectral_apply; every bit defined by include/karma.h).  Returns
    float64 (n, p)."""
    device, n, nnz, indptr, indices, weights = _csr_graph(graph)
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2 or x.shape[0] != n or not 1 <= x.shape[1] <= 32:
        raise ValueError(f"x must have shape ({n}, p) with 1 <= p <= 32, not {x.shape}")
    if n < 2:
        raise ValueError(f"need n >= 2, not {n}")
    if ctx is None:
        ctx = indptr.ctx if device else _lib.default_context()
    pp, keep_p = _dev_or_host(indptr, np.int64)
    pi, keep_i = _dev_or_host(indices, np.int32)
    pw, keep_w = _dev_or_host(weights, np.float64)
    out = np.empty_like(x)
    call("karma_spectral_apply", ctx.h, pp, pi, pw, n, nnz, 1 if device else 0, ptr(x), x.shape[1], ptr(out), 0)
    return out


class SpectralStats:
    """What umap_spectral(with_stats=True) returns beside y: vec, lam, res
    (float64 (n, dim)), comp (int32[n]) and the counts of info."""

    def __init__(self, vec, lam, res, comp, info):
        self.vec, self.lam, self.res, self.comp = vec, lam, res, comp
        self.components, self.not_converged, self.outer_rounds, self.applications = (int(v) for v in info)


def umap_spectral(graph, n_components, seed, tol=1e-4, max_outer=100, ctx=None, out_device=False, with_stats=False):
    """UMAP's spectral start of a symmetric CSR graph, component by component
    (karma_umap_spectral; the contract is in include/karma.h): graph =
    (indptr, indices, weights) as umap_graph returns them, numpy arrays or
    DevBufs.  Returns y float64 (n, n_components) for umap_layout's init= (a
    numpy array, or a DevBuf with out_device=True); with_stats=True returns
    (y, SpectralStats).  tol: the residual |S v - theta v| below which a
    component's eigenvectors count as converged (umap's eigsh tolerance);
    max_outer: the outer rounds a component may take.  A component that does
    not converge takes the random start on its rows and is counted in the
    stats; it is not an error."""
    device, n, nnz, indptr, indices, weights = _csr_graph(graph)
    dim, seed, tol, max_outer = int(n_components), int(seed), float(tol), int(max_outer)
    if n < 2:
        raise ValueError(f"need n >= 2, not {n}")
    if not 1 <= dim <= 16:
        raise ValueError(f"need 1 <= n_components <= 16, not {dim}")
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError(f"need tol finite and > 0, not {tol}")
    if max_outer < 1:
        raise ValueError(f"need max_outer >= 1, not {max_outer}")
    if ctx is None:
        ctx = indptr.ctx if device else _lib.default_context()
    pp, keep_p = _dev_or_host(indptr, np.int64)
    pi, keep_i = _dev_or_host(indices, np.int32)
    pw, keep_w = _dev_or_host(weights, np.float64)

    def make(shape, dtype):
        return _lib.DevBuf(ctx, shape, dtype) if out_device else np.empty(shape, dtype)

    def arg(buf):
        return None if buf is None else (ctypes.c_void_p(buf.ptr) if out_device else ptr(buf))

    y = make((n, dim), np.float64)
    vec = lam = res = comp = None
    if with_stats:
        vec, lam, res = (make((n, dim), np.float64) for _ in range(3))
        comp = make((n,), np.int32)
    info = np.zeros(4, np.int64)
    call("karma_umap_spectral", ctx.h, pp, pi, pw, n, nnz, 1 if device else 0, dim, ctypes.c_uint64(seed & (2**64 - 1)),
         tol, max_outer, arg(y), arg(vec), arg(lam), arg(res), arg(comp), 1 if out_device else 0, ptr(info))
    if info[1]:
        logger.warning(f"Spectral initialisation: {int(info[1])} of {int(info[0])} graph components did not converge "
                       f"within {max_outer} rounds; they start from random coordinates.")
    return (y, SpectralStats(vec, lam, res, comp, info)) if with_stats else y


def umap(x, n_neighbors=15, n_components=2, min_dist=0.1, spread=1.0, random_state=42, n_epochs=None, init=None,
         knn=None, ctx=None):
    """UMAP of the rows of the float64 matrix x (n, M) on the device: exact
    neighbour lists (knn_rows, or the (idx, dist) passed as knn=), the fuzzy
    graph (umap_graph), the curve (umap_ab) and the layout (umap_layout) from a
    random start (or init=: an array, or "spectral" for umap_spectral's start,
    built on the device and handed over there).  x: what knn_rows accepts, a
    DeviceProfile included; the lists and the graph stay on the device.
    n_epochs=None: 500 for n <= 10000, else 200.  Returns float64[n,
    n_components].  Every bit is defined by include/karma.h; the result is not
    claimed to equal umap-learn's coordinates (its layout is a racy parallel
    SGD with its own generator)."""
    host, _, n, _, _ = _knn_source(x)
    if isinstance(init, str) and init not in ("spectral", "random"):
        raise ValueError(f"init must be None, \"random\", \"spectral\" or an array, not {init!r}")
    if isinstance(init, str) and init == "random":
        init = None
    if ctx is None:
        ctx = x.ctx if host is None else _lib.default_context()
    own = []
    try:
        if knn is None:
            idx, dist = knn_rows(x, n_neighbors, ctx=ctx, out_device=True)
            own += [idx, dist]
        else:
            idx, dist = knn
            if not _on_device(idx, dist):
                idx = _lib.DevBuf.from_numpy(ctx, np.ascontiguousarray(idx, np.int32))
                dist = _lib.DevBuf.from_numpy(ctx, np.ascontiguousarray(dist, np.float64))
                own += [idx, dist]
            if tuple(idx.shape) != (n, int(n_neighbors)) or tuple(dist.shape) != tuple(idx.shape):
                raise ValueError(f"knn must be (idx, dist) of shape ({n}, {int(n_neighbors)}), not {idx.shape}")
        graph = umap_graph(idx, dist, ctx=ctx, out_device=True)
        own.append(graph[0])  # indices and weights are views of buffers that close with them
        own += [g._owner for g in graph[1:]]
        a, b = umap_ab(spread, min_dist)
        epochs = umap_default_epochs(n) if n_epochs is None else int(n_epochs)
        seed = 0 if random_state is None else int(random_state)
        if isinstance(init, str):  # "spectral": the start is built where the graph lies and stays there
            start = umap_spectral(graph, n_components, seed, ctx=ctx, out_device=True)
            own.append(start)
            return umap_layout(graph, n_components, a, b, epochs, seed, init=start, ctx=ctx).numpy()
        return umap_layout(graph, n_components, a, b, epochs, seed, init=init, ctx=ctx)
    finally:
        for buf in own:
            buf.close()


KNN_MAX_INDEX = (1 << 31) - 1  # cand_base + nc may reach it (include/karma.h, karma_knn_block)


def _knn_k(k):
    k = int(k)
    k_max = _lib.knn_tile()[3]
    if k < 1 or k > k_max:
        raise ValueError(f"need 1 <= k <= {k_max}, not k = {k}")
    return k


class KnnState:
    """Per-query neighbour lists that outlive a call (karma_knn_block; the
    contract is in include/karma.h): nq rows of the k smallest (d2 bits,
    index) seen so far, on the device.  update() folds one block of candidate
    rows with a global index base into them, in any block order; merge() folds
    another state of the same queries; finish() gives (idx, dist) as knn_rows
    does.  No candidate index may be offered twice.  The buffers are allocated
    at the first update."""

    def __init__(self, ctx, nq, k):
        nq = int(nq)
        if nq < 0 or nq >= 1 << 31:
            raise ValueError(f"need 0 <= nq < 2^31, not nq = {nq}")
        self.ctx, self.nq, self.k = ctx, nq, _knn_k(k)
        self.keys = self.idx = None
        self.first = True  # nothing folded yet: the next update does not read the state
        self.rows_seen = 0  # candidate rows offered so far
        self.closed = False

    def _buffers(self):
        if self.keys is None:
            self.keys = _lib.DevBuf(self.ctx, (self.nq, self.k), np.uint64)
            self.idx = _lib.DevBuf(self.ctx, (self.nq, self.k), np.int32)

    def _open(self):
        if self.closed:
            raise ValueError("KnnState is closed")

    def update(self, q, c, cand_base, cand_split=0):
        """Fold the candidate rows c (index of row r: cand_base + r) into the
        lists of the query rows q.  q, c: a numpy array, a DevBuf or a
        DeviceProfile of the same column count; q has the state's nq rows.
        cand_split: 0 lets the library choose, S >= 1 runs S slices of the
        candidate tiles side by side (the lists do not depend on it)."""
        self._open()
        qh, qd, nq, M, ldq = _knn_source(q)
        ch, cd, nc, Mc, ldc = _knn_source(c)
        cand_base, cand_split = int(cand_base), int(cand_split)
        if nq != self.nq:
            raise ValueError(f"the state holds {self.nq} query rows, not {nq}")
        if M != Mc:
            raise ValueError(f"queries and candidates must have the same columns, not {M} and {Mc}")
        if cand_base < 0 or cand_base + nc > KNN_MAX_INDEX:
            raise ValueError(f"need 0 <= cand_base and cand_base + nc <= 2^31 - 1, not {cand_base} + {nc}")
        if cand_split < 0:
            raise ValueError(f"cand_split must not be negative, not {cand_split}")
        if self.nq and (nc or self.first):
            self._buffers()
            call("karma_knn_block", self.ctx.h, ctypes.c_void_p(qd) if qh is None else ptr(qh), nq, ldq,
                 1 if qh is None else 0, ctypes.c_void_p(cd) if ch is None else ptr(ch), nc, ldc,
                 1 if ch is None else 0, M, cand_base, self.k, ctypes.c_void_p(self.keys.ptr),
                 ctypes.c_void_p(self.idx.ptr), 1, 1 if self.first else 0, cand_split)
        self.first = False
        self.rows_seen += nc

    def merge(self, other):
        """Fold another state of the same queries (same nq, k and context) into this one."""
        self._open()
        if not isinstance(other, KnnState):
            raise TypeError(f"merge takes a KnnState, not {type(other).__name__}")
        other._open()
        if (other.nq, other.k) != (self.nq, self.k):
            raise ValueError(f"the states differ: {self.nq} x {self.k} and {other.nq} x {other.k}")
        if other is self:
            raise ValueError("a state cannot be merged into itself (no index may be offered twice)")
        if other.first:
            return
        if self.nq:
            self._buffers()
            if self.first:  # nothing here yet: the other's lists as they are
                self.keys.copy_from_device(other.keys)
                self.idx.copy_from_device(other.idx)
            else:
                call("karma_knn_merge", self.ctx.h, ctypes.c_void_p(self.keys.ptr), ctypes.c_void_p(self.idx.ptr),
                     ctypes.c_void_p(other.keys.ptr), ctypes.c_void_p(other.idx.ptr), self.nq, self.k, 1)
        self.first = False
        self.rows_seen += other.rows_seen

    def finish(self, out_device=False):
        """(idx int32[nq, k], dist float64[nq, k]): numpy arrays, or DevBufs
        with out_device=True.  Fewer than k candidate rows so far is an error."""
        self._open()
        if self.rows_seen < self.k:
            raise ValueError(f"need 1 <= k <= the candidate rows offered, not k = {self.k} with {self.rows_seen} rows")
        if out_device:
            idx, dist = _lib.DevBuf(self.ctx, (self.nq, self.k), np.int32), \
                _lib.DevBuf(self.ctx, (self.nq, self.k), np.float64)
            pi, pd = ctypes.c_void_p(idx.ptr), ctypes.c_void_p(dist.ptr)
        else:
            idx, dist = np.empty((self.nq, self.k), np.int32), np.empty((self.nq, self.k), np.float64)
            pi, pd = ptr(idx), ptr(dist)
        if self.nq:
            call("karma_knn_finish", self.ctx.h, ctypes.c_void_p(self.keys.ptr), ctypes.c_void_p(self.idx.ptr),
                 self.nq, self.k, 1, pi, pd, 1 if out_device else 0)
        return idx, dist

    def close(self):
        for b in (self.keys, self.idx):
            if b is not None:
                b.close()
        self.keys = self.idx = None
        self.closed = True


def knn_blocked(x, k, block_rows, ctx=None):
    """knn_rows(x, k) of a host matrix (a numpy array, a numpy.memmap) walked
    in blocks of block_rows rows: one query block, one candidate block and the
    query block's lists are on the device at a time, so x may be larger than
    device memory.  Returns (idx int32[n, k], dist float64[n, k]), bit for bit
    knn_rows' result."""
    if not isinstance(x, np.ndarray):
        raise TypeError(f"the matrix must be a host numpy array (or memmap), not {type(x).__name__}")
    if x.dtype != np.float64:
        raise TypeError(f"the matrix must be float64 (distances are defined on its bits), not {x.dtype}")
    if x.ndim != 2:
        raise ValueError(f"the matrix must have shape (n, M), not {x.shape}")
    n = x.shape[0]
    k, block_rows = int(k), int(block_rows)
    k_max = _lib.knn_tile()[3]
    if k < 1 or k > min(n, k_max):
        raise ValueError(f"need 1 <= k <= min(n, {k_max}), not k = {k} with n = {n}")
    if block_rows < 1:
        raise ValueError(f"block_rows must be at least 1, not {block_rows}")
    ctx = ctx or _lib.default_context()
    idx, dist = np.empty((n, k), np.int32), np.empty((n, k), np.float64)
    for lo in range(0, n, block_rows):
        hi = min(n, lo + block_rows)
        q = _lib.DevBuf.from_numpy(ctx, x[lo:hi])
        state = KnnState(ctx, hi - lo, k)
        try:
            for clo in range(0, n, block_rows):
                chi = min(n, clo + block_rows)
                c = q if clo == lo else _lib.DevBuf.from_numpy(ctx, x[clo:chi])
                try:
                    state.update(q, c, clo)
                finally:
                    if c is not q:
                        c.close()
            idx[lo:hi], dist[lo:hi] = state.finish()
        finally:
            state.close()
            q.close()
    return idx, dist


# ---------------------------------------------------------------------------
# Graph
# ---------------------------------------------------------------------------

class GraphJob:
    """An open karma_graph_records_begin call (one per context)."""

    def __init__(self, pairs_cls, ctx, h):
        self.pairs_cls, self.ctx, self.h = pairs_cls, ctx, h

    def end(self):
        h, self.h = self.h, None
        out = ctypes.c_void_p()
        call("karma_graph_records_end", h, ctypes.byref(out))
        return self.pairs_cls(self.ctx, out)

    def __del__(self):
        if getattr(self, "h", None):  # never ended: end it (frees the job and its list)
            try:
                self.end().close()
            except Exception:
                pass


class FlaggedRecords:
    """KARMA_REC_FLAGGED words in device memory, made by flag_records_device
    (karma_records_flag).  Owns its buffer: keep it alive while a job reads it.
    .ptr: the device address, .n_records: the word count, .n_reads: the number
    of flag bits set, .to_host(): the words as a uint32 array."""

    def __init__(self, ctx, buf, n_records, n_reads):
        self.ctx, self._buf, self.n_records, self.n_reads = ctx, buf, int(n_records), int(n_reads)

    @property
    def ptr(self):
        return self._buf.ptr

    def to_host(self):
        return self._buf.numpy()[: self.n_records]

    def close(self):
        if self._buf is not None:
            self._buf.close()
            self._buf = None


def _pairs_array(records):
    """Host records as a C-order uint32[n, 2] array (ValueError / TypeError otherwise)."""
    a = np.asarray(records)
    if a.size == 0:
        return np.zeros((0, 2), np.uint32)
    if a.dtype.kind not in "iu":
        raise TypeError(f"records must be integers (uint32 read and contig ids), not {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"records must have shape (n, 2): (read id, contig id) rows, not {a.shape}")
    if a.dtype != np.uint32 and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise ValueError("read and contig ids must fit 32 unsigned bits")
    return np.ascontiguousarray(a, dtype=np.uint32)


def flag_records_device(records=None, *, device_ptr=None, n_records=None, grouped=True, ctx=None):
    """(read, contig) records -> KARMA_REC_FLAGGED words in device memory
    (karma_records_flag): the device twin of flag_records, for records on the
    host (records: uint32[n, 2]) or already in HBM (device_ptr, n_records).
    grouped=True: read ids must not decrease (KarmaError, KARMA_ERR_UNSORTED);
    grouped=False: any order, stably sorted by read id on the device first.
    A contig id >= 2^31 is a KarmaError (KARMA_ERR_ARG).  Returns FlaggedRecords."""
    if (records is None) == (device_ptr is None):
        raise ValueError("give either records (a host array) or device_ptr (with n_records)")
    fmt = _lib.KARMA_REC_SORTED if grouped else _lib.KARMA_REC_UNSORTED
    if device_ptr is not None:
        if n_records is None:
            raise ValueError("device_ptr needs n_records")
        n = int(n_records)
        if n < 0:
            raise ValueError("n_records must not be negative")
        src, on_device = ctypes.c_void_p(int(device_ptr)), 1
    else:
        if n_records is not None:
            raise ValueError("n_records goes with device_ptr; host records carry their own length")
        rec = _pairs_array(records)
        n = len(rec)
        src, on_device = (ptr(rec) if n else None), 0
    ctx = ctx or _lib.default_context()
    buf = _lib.DevBuf(ctx, (max(n, 1),), np.uint32)
    reads = ctypes.c_int64(0)
    try:
        call("karma_records_flag", ctx.h, src, n, fmt, on_device, ctypes.c_void_p(buf.ptr), 1, ctypes.byref(reads))
    except Exception:
        buf.close()
        raise
    return FlaggedRecords(ctx, buf, n, reads.value)


class Pairs:
    """Sorted unique (a << 32 | b, count) list (karma_pairs)."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    @classmethod
    def from_records(cls, ctx, records, n_contigs, grouped=True, device_ptr=None, n_records=None, flagged=False):
        """flagged: the records are KARMA_REC_FLAGGED words (flag_records), one u32 each.
        A FlaggedRecords (flag_records_device) may stand for records or device_ptr."""
        h = ctypes.c_void_p()
        fr = device_ptr if isinstance(device_ptr, FlaggedRecords) else records
        if isinstance(fr, FlaggedRecords):
            device_ptr, n_records, flagged = fr.ptr, fr.n_records, True
        flags = _lib.KARMA_REC_FLAGGED if flagged else _lib.KARMA_REC_SORTED if grouped else _lib.KARMA_REC_UNSORTED
        if device_ptr is not None:
            call("karma_graph_records", ctx.h, ctypes.c_void_p(device_ptr), n_records, n_contigs, flags, 1,
                 ctypes.byref(h))
        else:
            rec = np.ascontiguousarray(records, dtype=np.uint32)
            rec = rec.reshape(-1) if flagged else rec.reshape(-1, 2)
            call("karma_graph_records", ctx.h, ptr(rec) if len(rec) else None, len(rec), n_contigs, flags, 0,
                 ctypes.byref(h))
        return cls(ctx, h)

    @classmethod
    def from_records_begin(cls, ctx, n_contigs, device_ptr, n_records=None, grouped=True, split_bounds=None,
                           flagged=False):
        """First half of from_records on device records (karma_graph_records_begin):
        the pipeline is enqueued up to its host synchronisation; .end() finishes.
        device_ptr: a device address (with n_records), or a FlaggedRecords.
        split_bounds: owner bounds the list will be split at (karma_graph_split_hint)."""
        keep = None
        if isinstance(device_ptr, FlaggedRecords):  # n_records may be None: the words' own count
            keep = device_ptr
            device_ptr, n_records, flagged = keep.ptr, keep.n_records, True
        if split_bounds is not None:
            b = np.ascontiguousarray(split_bounds, np.int64)
            call("karma_graph_split_hint", ctx.h, ptr(b), len(b) - 1)
        h = ctypes.c_void_p()
        flags = _lib.KARMA_REC_FLAGGED if flagged else _lib.KARMA_REC_SORTED if grouped else _lib.KARMA_REC_UNSORTED
        call("karma_graph_records_begin", ctx.h, ctypes.c_void_p(device_ptr), n_records, n_contigs, flags, 1,
             ctypes.byref(h))
        job = GraphJob(cls, ctx, h)
        job.records = keep  # the words stay alive until the job ends
        return job

    @classmethod
    def from_eq(cls, ctx, cls_off, members, counts, pair_skip, n_contigs):
        h = ctypes.c_void_p()
        cls_off = np.ascontiguousarray(cls_off, np.int64)
        members = np.ascontiguousarray(members, np.uint32)
        counts = np.ascontiguousarray(counts, np.int64)
        skip = np.ascontiguousarray(pair_skip, np.uint8)
        call("karma_graph_eq", ctx.h, ptr(cls_off), ptr(members) if len(members) else None,
             ptr(counts) if len(counts) else None, ptr(skip) if len(skip) else None, len(cls_off) - 1, n_contigs, 0,
             ctypes.byref(h))
        return cls(ctx, h)

    @classmethod
    def from_eq_compact(cls, ctx, sizes, members, counts32, n_contigs):
        """karma_graph_eq_compact: sizes uint8[C] (member count | 0x80 for the
        size token "1"), members uint32, counts uint32[C]."""
        h = ctypes.c_void_p()
        sizes = np.ascontiguousarray(sizes, np.uint8)
        members = np.ascontiguousarray(members, np.uint32)
        counts32 = np.ascontiguousarray(counts32, np.uint32)
        call("karma_graph_eq_compact", ctx.h, ptr(sizes) if len(sizes) else None,
             ptr(members) if len(members) else None, len(members), ptr(counts32) if len(counts32) else None,
             len(sizes), n_contigs, ctypes.byref(h))
        return cls(ctx, h)

    @classmethod
    def merge_runs_kc(cls, ctx, kc_dev_ptr, runs):
        """Merge received runs of interleaved (key, count) int64 pairs in device memory."""
        off = np.zeros(len(runs) + 1, np.int64)
        np.cumsum(np.asarray(runs, np.int64), out=off[1:])
        h = ctypes.c_void_p()
        call("karma_pairs_merge_runs_kc", ctx.h, ctypes.c_void_p(kc_dev_ptr) if kc_dev_ptr else None, ptr(off),
             len(runs), ctypes.byref(h))
        return cls(ctx, h)

    def get_kc(self, kc_dev_ptr):
        """Interleaved (key, count) int64 pairs into device memory (stream-ordered)."""
        call("karma_pairs_get_kc", self.h, ctypes.c_void_p(kc_dev_ptr) if kc_dev_ptr else None)

    @classmethod
    def merge(cls, ctx, keys, counts, device=False, n=None, runs=None):
        """Sorted unique (key, count) list.  runs = lengths of consecutive runs that
        are each sorted by key (an exchange owner's received slices): merged by a
        merge tree instead of a full sort."""
        h = ctypes.c_void_p()
        if runs is not None:
            if device:
                # the run offsets as a ctypes array (no numpy on this per-step path)
                off = (ctypes.c_int64 * (len(runs) + 1))(0, *itertools.accumulate(int(r) for r in runs))
                assert n is None or n == off[len(runs)], "run lengths do not add up to n"
                call("karma_pairs_merge_runs", ctx.h, ctypes.c_void_p(keys) if keys else None,
                     ctypes.c_void_p(counts) if counts else None, off, len(runs), 1, ctypes.byref(h))
                return cls(ctx, h)
            off = np.zeros(len(runs) + 1, np.int64)
            np.cumsum(np.asarray(runs, np.int64), out=off[1:])
            keys = np.ascontiguousarray(keys, np.uint64)
            counts = np.ascontiguousarray(counts, np.int64)
            call("karma_pairs_merge_runs", ctx.h, ptr(keys) if len(keys) else None,
                 ptr(counts) if len(counts) else None, ptr(off), len(runs), 0, ctypes.byref(h))
            return cls(ctx, h)
        if device:
            call("karma_pairs_merge", ctx.h, ctypes.c_void_p(keys) if keys else None,
                 ctypes.c_void_p(counts) if counts else None, n, 1, ctypes.byref(h))
        else:
            keys = np.ascontiguousarray(keys, np.uint64)
            counts = np.ascontiguousarray(counts, np.int64)
            call("karma_pairs_merge", ctx.h, ptr(keys) if len(keys) else None, ptr(counts) if len(counts) else None,
                 len(keys), 0, ctypes.byref(h))
        return cls(ctx, h)

    def count(self):
        n = ctypes.c_int64()
        call("karma_pairs_count", self.h, ctypes.byref(n))
        return n.value

    def device_ptrs(self):
        k, c = ctypes.c_void_p(), ctypes.c_void_p()
        call("karma_pairs_device", self.h, ctypes.byref(k), ctypes.byref(c))
        return k.value, c.value

    def get(self):
        n = self.count()
        keys = np.zeros(max(n, 1), np.uint64)
        counts = np.zeros(max(n, 1), np.int64)
        first = np.zeros(max(n, 1), np.uint64)
        call("karma_pairs_get", self.h, ptr(keys), ptr(counts), ptr(first), 0)
        return keys[:n], counts[:n], first[:n]

    def split(self, bounds):
        bounds = np.ascontiguousarray(bounds, np.int64)
        starts = np.zeros(len(bounds), np.int64)
        call("karma_pairs_split", self.h, ptr(bounds), len(bounds) - 1, ptr(starts))
        return starts

    def split_kc(self, bounds, kc_dev_ptr):
        """split(bounds) and get_kc(kc_dev_ptr) in one launch (karma_pairs_split_kc)."""
        bounds = np.ascontiguousarray(bounds, np.int64)
        starts = np.zeros(len(bounds), np.int64)
        call("karma_pairs_split_kc", self.h, ptr(bounds), len(bounds) - 1, ptr(starts),
             ctypes.c_void_p(kc_dev_ptr) if kc_dev_ptr else None)
        return starts

    def edges_begin(self, mode, n_contigs):
        """First half of edges() (karma_edges_begin): returns the open Edges and the
        device address of its int64[n_contigs] totals, for an all-gather before
        Edges.end() computes the weights."""
        h = ctypes.c_void_p()
        tp = ctypes.c_void_p()
        call("karma_edges_begin", self.ctx.h, self.h, mode, n_contigs, ctypes.byref(h), ctypes.byref(tp))
        e = Edges(self.ctx, h, -1, n_contigs)
        e._pairs = self  # the list stays alive until end()
        return e, tp.value

    def totals_device(self, dst_dev_ptr, n_contigs):
        call("karma_pairs_totals", self.h, ctypes.c_void_p(dst_dev_ptr), n_contigs)

    def edges(self, mode, n_contigs, totals_dev_ptr=None):
        h = ctypes.c_void_p()
        E = ctypes.c_int64()
        call("karma_edges_from_pairs", self.ctx.h, self.h, mode,
             ctypes.c_void_p(totals_dev_ptr) if totals_dev_ptr else None, n_contigs, ctypes.byref(h),
             ctypes.byref(E))
        return Edges(self.ctx, h, E.value, n_contigs)

    def rebind(self, ctx):
        """Run later kernels on this list on ``ctx``'s stream (karma_pairs_rebind)."""
        call("karma_pairs_rebind", self.h, ctx.h)
        self.ctx = ctx

    def close(self):
        if getattr(self, "h", None):
            _lib.load().karma_pairs_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


@dataclass
class EdgeArrays:
    a: np.ndarray
    b: np.ndarray
    shared: np.ndarray
    weight: np.ndarray
    first: np.ndarray
    totals: np.ndarray


class Edges:
    def __init__(self, ctx, h, E, n_contigs):
        self.ctx, self.h, self._E, self.n_contigs = ctx, h, E, n_contigs

    @property
    def E(self):
        """Edge count; after end(count=False) its first read synchronises and
        reports the edge stage's errors (karma_edges_count)."""
        if self._E is None:
            E = ctypes.c_int64()
            call("karma_edges_count", self.h, ctypes.byref(E))
            self._E = E.value
        return self._E

    def end(self, count=True):
        """Second half of Pairs.edges_begin (karma_edges_end): weights, and the
        edge count (count=False: launched only; E is read when first used)."""
        if count:
            E = ctypes.c_int64()
            call("karma_edges_end", self.h, ctypes.byref(E))
            self._E = E.value
        else:
            call("karma_edges_end", self.h, None)
            self._E = None
        self._pairs = None
        return self

    def get(self) -> EdgeArrays:
        """The edges in host arrays (pinned host memory: the copies run at the
        full PCIe rate; the blocks return to the library's cache with the arrays)."""
        E = self.E
        e1, n1 = max(E, 1), max(self.n_contigs, 1)
        # one pinned block: s, w, f, totals (8-byte items) then a, b (4-byte)
        blk = _lib.pinned_empty(8 * (3 * e1 + n1) + 4 * (2 * e1 + 1), np.uint8)
        o = [0]

        def take(n, dt):
            dt = np.dtype(dt)
            v = blk[o[0]:o[0] + n * dt.itemsize].view(dt)
            o[0] += n * dt.itemsize
            return v
        s, w, f, t = take(e1, np.int64), take(e1, np.float64), take(e1, np.uint64), take(n1, np.int64)
        a, b = take(e1, np.uint32), take(e1, np.uint32)
        call("karma_edges_get_all", self.h, ptr(a), ptr(b), ptr(s), ptr(w), ptr(f), ptr(t), 0)
        return EdgeArrays(a[:E], b[:E], s[:E], w[:E], f[:E], t[: self.n_contigs])

    def get_ordered(self):
        """Eq edge stages: (a, b, w) in the reference's insertion order -- by a,
        then by the pair's first emission (read_graph.py:96-131), ordered on the
        device (karma_edges_get_ordered); one pinned block."""
        E = self.E
        e1 = max(E, 1)
        blk = _lib.pinned_empty(16 * e1, np.uint8)
        w = blk[: 8 * e1].view(np.float64)
        a = blk[8 * e1: 12 * e1].view(np.uint32)
        b = blk[12 * e1:].view(np.uint32)
        call("karma_edges_get_ordered", self.h, ptr(a), ptr(b), ptr(w), 0)
        return a[:E], b[:E], w[:E]

    def close(self):
        if getattr(self, "h", None):
            _lib.load().karma_edges_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def graph_from_records(records, n_contigs, grouped=True, ctx=None, flagged=False) -> EdgeArrays:
    """Shared-read edges from (read, contig) records (read_graph.py:19-50 semantics);
    flagged: records given as flag_records words."""
    ctx = ctx or _lib.default_context()
    p = Pairs.from_records(ctx, records, n_contigs, grouped=grouped, flagged=flagged)
    try:
        e = p.edges(_lib.KARMA_MODE_READS, n_contigs)
        try:
            return e.get()
        finally:
            e.close()
    finally:
        p.close()


def graph_from_eq(cls_off, members, counts, pair_skip, n_contigs, ctx=None) -> EdgeArrays:
    """Eq-class edges (read_graph.py:86-131 semantics), with first-emission order."""
    ctx = ctx or _lib.default_context()
    p = Pairs.from_eq(ctx, cls_off, members, counts, pair_skip, n_contigs)
    try:
        e = p.edges(_lib.KARMA_MODE_EQ, n_contigs)
        try:
            return e.get()
        finally:
            e.close()
    finally:
        p.close()


def graph_from_eq_ordered(cls_off, members, counts, pair_skip, n_contigs, ctx=None):
    """Eq-class edges as the drop-in needs them: (a, b, w) in the reference's
    insertion order (read_graph.py:96-131), ordered on the device."""
    ctx = ctx or _lib.default_context()
    p = Pairs.from_eq(ctx, cls_off, members, counts, pair_skip, n_contigs)
    try:
        e = p.edges(_lib.KARMA_MODE_EQ, n_contigs)
        try:
            return e.get_ordered()
        finally:
            e.close()
    finally:
        p.close()


def eq_compact(cls_off, counts, pair_skip):
    """(sizes uint8, counts uint32) of wide eq arrays for karma_graph_eq_compact,
    or None when a class has > 127 members or a count past 2^32 - 1 (the form
    the C++ parser emits directly, ingest.parse_eq(compact=True))."""
    m = np.diff(np.asarray(cls_off, np.int64))
    counts = np.asarray(counts, np.int64)
    if len(m) and (m.max() > 127 or counts.min() < 0 or counts.max() > 0xFFFFFFFF):
        return None
    sizes = m.astype(np.uint8)
    if pair_skip is not None and len(pair_skip):
        sizes |= (np.asarray(pair_skip, np.uint8) != 0).astype(np.uint8) << 7
    return sizes, counts.astype(np.uint32)


def graph_from_eq_compact_ordered(sizes, members, counts32, n_contigs, ctx=None):
    """graph_from_eq_ordered from the compact inputs (karma_graph_eq_compact)."""
    ctx = ctx or _lib.default_context()
    p = Pairs.from_eq_compact(ctx, sizes, members, counts32, n_contigs)
    try:
        e = p.edges(_lib.KARMA_MODE_EQ, n_contigs)
        try:
            return e.get_ordered()
        finally:
            e.close()
    finally:
        p.close()


# ---------------------------------------------------------------------------
# Synthetic inputs through the native generator (twin of synth.py)
# ---------------------------------------------------------------------------

def synth_contigs(seed, n, len_min=400, len_span=800, n_rate=0, first=0):
    """(blob uint8, offsets int64[n+1], key_len int32[n]) of contigs ">ctg<i>",
    i in [first, first + n) of the global synthetic set (counter-based, so a
    shard generates only its own rows)."""
    lens = np.zeros(first + n, np.int64)
    call("karma_synth_contig_lengths", seed, first + n, len_min, len_span, ptr(lens))
    goffs = np.zeros(first + n + 1, np.int64)
    np.cumsum(lens, out=goffs[1:])
    gslice = np.ascontiguousarray(goffs[first:])
    blob = np.zeros(int(gslice[-1] - gslice[0]) + 16, np.uint8)
    call("karma_synth_contig_bases", seed, ptr(gslice), n, n_rate, ptr(blob))
    offs = gslice - gslice[0]
    key_len = _key_lens(first + n)[first:].copy()
    return blob, offs, key_len


def _key_lens(n):
    i = np.arange(n)
    digits = np.ones(n, np.int32)
    p = 10
    while p <= n:
        digits += (i >= p)
        p *= 10
    return (4 + digits).astype(np.int32)


def synth_genes(seed, n_contigs, gene_max=4):
    ng = ctypes.c_int64()
    call("karma_synth_n_genes", seed, n_contigs, gene_max, ctypes.byref(ng))
    gf = np.zeros(ng.value, np.int64)
    gs = np.zeros(ng.value, np.int32)
    call("karma_synth_genes", seed, n_contigs, gene_max, ptr(gf), ptr(gs))
    return gf, gs


def flag_records(records):
    """(read, contig) records grouped by read -> KARMA_REC_FLAGGED words (the
    read ids replaced by read-start flags): contig | (first record of its read) << 31.
    The graph depends only on which records share a read, so the two formats
    give the same graph.  Read ids that decrease (records not grouped by read:
    ids A, B, A would become three reads) are a ValueError, the condition the
    pairs format reports as KARMA_ERR_UNSORTED; the flagged words themselves no
    longer carry the ids, so nothing downstream can check it."""
    rec = np.asarray(records, np.uint32).reshape(-1, 2)
    if len(rec) and int(rec[:, 1].max()) >= 1 << 31:
        raise ValueError("flagged records hold contig ids < 2^31")
    if len(rec) > 1 and bool((rec[1:, 0] < rec[:-1, 0]).any()):
        raise ValueError("records are not grouped by read (read ids decrease)")
    out = rec[:, 1].copy()
    if len(rec):
        start = np.empty(len(rec), np.uint32)
        start[0] = 1
        np.not_equal(rec[1:, 0], rec[:-1, 0], out=start[1:], casting="unsafe")
        out |= start << np.uint32(31)
    return out


def synth_records(seed, n_contigs, frag_lo, frag_hi, paired, gene_max=4, genes=None):
    """records uint32[A, 2] (read, contig) for fragments [frag_lo, frag_hi)."""
    gf, gs = genes if genes is not None else synth_genes(seed, n_contigs, gene_max)
    nf = frag_hi - frag_lo
    cnt = np.zeros(max(nf, 1), np.int32)
    call("karma_synth_read_counts", seed, ptr(gf), ptr(gs), len(gf), frag_lo, frag_hi, int(paired), ptr(cnt))
    off = np.zeros(nf + 1, np.int64)
    np.cumsum(cnt[:nf], out=off[1:])
    rec = np.zeros((max(int(off[-1]), 1), 2), np.uint32)
    call("karma_synth_read_records", seed, ptr(gf), ptr(gs), len(gf), frag_lo, frag_hi, int(paired), ptr(off),
         ptr(rec))
    return rec[: int(off[-1])]


def synth_eq_classes(seed, n_contigs, frag_lo, frag_hi, paired, gene_max=4, genes=None):
    """(cls_off int64[C+1], members uint32[], counts int64[C]) of the fragments'
    eq classes, first-seen order (native twin of synth.eq_classes)."""
    gf, gs = genes if genes is not None else synth_genes(seed, n_contigs, gene_max)
    nc, nm = ctypes.c_int64(), ctypes.c_int64()
    call("karma_synth_eq_classes", seed, ptr(gf), ptr(gs), len(gf), frag_lo, frag_hi, int(paired), ctypes.byref(nc),
         ctypes.byref(nm), None, None, None)
    off = np.zeros(nc.value + 1, np.int64)
    mem = np.zeros(max(nm.value, 1), np.uint32)
    cnt = np.zeros(max(nc.value, 1), np.int64)
    call("karma_synth_eq_classes", seed, ptr(gf), ptr(gs), len(gf), frag_lo, frag_hi, int(paired), ctypes.byref(nc),
         ctypes.byref(nm), ptr(off), ptr(mem), ptr(cnt))
    return off, mem[: nm.value], cnt[: nc.value]
