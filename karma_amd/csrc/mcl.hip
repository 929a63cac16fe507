// mcl.hip — Markov clustering of a weighted graph on the device (karma_mcl,
// karma_adj_mcl).  Kernels "mcl_start" (validate, keys, column offsets,
// columns), "mcl_expand" (the general path's count, emit, run sums, select) and
// "mcl_iter" (the fused path: one launch per iteration).
//
// The contract (include/karma.h) defines every output bit: each sum is taken in
// a stated order, one IEEE operation at a time, so the two paths, any batch
// size and any launch order give the same matrix.  No floating-point atomics:
// the iteration's chaos is folded with an integer atomicMax on an
// order-preserving image of the f64's bits.
//
// The matrix.  The start matrix is a CSC whose columns are as wide as the
// nodes' degrees.  From the first iteration on every column holds at most
// R = resource entries, kept in a padded layout: column j at [j R, j R + len[j]),
// ascending by row.  Both layouts are read through Mat.
//
// The general path serves any width.  Per slot (entry k of column j) the
// candidates it will emit are counted (the length of column k) and scanned; the
// host reads the per-column offsets and cuts the columns into batches of at
// most cand_cap candidates.  Per batch: every slot writes its candidates
// (key = j << 32 | i, product) at its scanned place, that is in column order,
// then ascending k; the library's stable radix sort orders them by (j, i), and
// stability leaves equal keys in ascending k, the summation order; the head of
// each run of equal keys sums its run; a thread per column walks its heads,
// keeps the top R under (X descending, i ascending), prunes, normalises,
// inflates and writes the padded column.
//
// The fused path serves iterations >= 2 for R <= 8, where a column has at most
// R * R <= 64 candidates: a group of 16 lanes (R <= 4, a 4 x 4 square) or 64
// lanes (R <= 8, an 8 x 8 square, one wave) per column, one candidate per lane.
// The group ranks its candidates by (row, k order) through LDS, each run's head
// sums it left to right, the heads are ranked for the top R, a ballot compacts
// the kept ones and the column's few lanes normalise, inflate and write it into
// the other of two buffers.  A launch whose predecessor converged (or did not
// run) returns at once, so the host queues kMclQueue iterations between reads
// of their chaos words.
#include <algorithm>
#include <new>
#include <vector>

#include "karma_internal.h"
#include "mcl_args.h"
#include "umap_math.h"

using namespace karma;

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

// a matrix in either layout: CSC (cp != null) or padded (len, stride R)
struct Mat {
    const int64_t* cp;
    const int32_t* len;
    int R;
    const uint32_t* rows;
    const double* vals;
};
__device__ __forceinline__ int64_t mat_begin(const Mat& m, int64_t j) { return m.cp ? m.cp[j] : j * m.R; }
__device__ __forceinline__ int64_t mat_size(const Mat& m, int64_t j) {
    return m.cp ? m.cp[j + 1] - m.cp[j] : (int64_t)m.len[j];
}
// the column of slot e (n >= 1 columns) and whether the slot holds an entry
__device__ __forceinline__ int64_t mat_column(const Mat& m, int64_t n, int64_t e, bool* valid) {
    if (!m.cp) {
        const int64_t j = e / m.R;
        *valid = e - j * m.R < (int64_t)m.len[j];
        return j;
    }
    int64_t lo = 0, hi = n;  // the last j with cp[j] <= e
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (m.cp[mid] <= e) lo = mid; else hi = mid;
    }
    *valid = true;
    return lo;
}

// f64 -> u64 keeping the order (0 is below every image: "not written")
__host__ __device__ inline unsigned long long chaos_image(double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    const long long b = __double_as_longlong(c);
#else
    long long b;
    __builtin_memcpy(&b, &c, 8);
#endif
    return b < 0 ? ~(unsigned long long)b : (unsigned long long)b | 0x8000000000000000ull;
}
__host__ __device__ inline double chaos_value(unsigned long long u) {
    const unsigned long long b = (u & 0x8000000000000000ull) ? u & 0x7FFFFFFFFFFFFFFFull : ~u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double c;
    __builtin_memcpy(&c, &b, 8);
    return c;
#endif
}

__device__ __forceinline__ double mcl_inflate(double x, double inflation) {
    return inflation == 2.0 ? x * x : kpow(x, inflation);
}

// ---- start -----------------------------------------------------------------------------

enum : int { kBadOff = 1, kBadNbr = 2, kBadWeight = 4, kBadDup = 8 };

// a graph's contents, checked before anything is indexed with them
__global__ __launch_bounds__(kThreads) void mcl_validate_kernel(const int64_t* __restrict__ off,
                                                                const uint32_t* __restrict__ nbr,
                                                                const double* __restrict__ w, int64_t n, int64_t nnz,
                                                                int* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int flags = 0;
    if (t < n && (off[t + 1] < off[t] || off[t + 1] > nnz || off[t] < 0)) flags |= kBadOff;
    if (t == 0 && (off[0] != 0 || off[n] != nnz)) flags |= kBadOff;
    if (t < nnz) {
        const double v = w[t];
        if ((int64_t)nbr[t] >= n) flags |= kBadNbr;
        if (!(v > 0.0) || v == INFINITY) flags |= kBadWeight;
    }
    if (flags) atomicOr(bad, flags);
}

// keys j << 32 | i of the entries (self entries and bad rows: n << 32, past every column) and of the n loops
__global__ __launch_bounds__(kThreads) void mcl_start_keys_kernel(const int64_t* __restrict__ off,
                                                                  const uint32_t* __restrict__ nbr, int64_t n,
                                                                  int64_t nnz, uint64_t* __restrict__ keys) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nnz + n) return;
    if (t >= nnz) {
        const uint64_t j = (uint64_t)(t - nnz);
        keys[t] = j << 32 | j;
        return;
    }
    int64_t lo = 0, hi = n;  // the last j with off[j] <= t; in [0, n) whatever off holds
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid; else hi = mid;
    }
    const uint64_t i = nbr[t];
    keys[t] = ((int64_t)i < n && (int64_t)i != lo) ? (uint64_t)lo << 32 | i : (uint64_t)n << 32;
}

// the same (column, row) twice: equal neighbours in the sorted keys (a column's loop key is there once)
__global__ __launch_bounds__(kThreads) void mcl_dup_kernel(const uint64_t* __restrict__ skeys, int64_t total, int64_t n,
                                                           int* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < 1 || t >= total) return;
    const uint64_t k = skeys[t];
    if ((int64_t)(k >> 32) < n && skeys[t - 1] == k) atomicOr(bad, kBadDup);
}

// sorted keys -> column offsets: position t opens every column in (column of t - 1, column of t]
__global__ __launch_bounds__(kThreads) void mcl_colptr_kernel(const uint64_t* __restrict__ skeys, int64_t total,
                                                              int64_t n, int64_t* __restrict__ colptr) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t > total) return;
    const int64_t cur = t < total ? (int64_t)(skeys[t] >> 32) : n;
    const int64_t prev = t > 0 ? (int64_t)(skeys[t - 1] >> 32) : -1;
    for (int64_t r = prev + 1; r <= cur && r <= n; ++r) colptr[r] = t;
}

// column j of the start matrix: its entries by row, the loop with the column's maximum, divided by the in-order sum
__global__ __launch_bounds__(kThreads) void mcl_start_cols_kernel(const uint64_t* __restrict__ skeys,
                                                                  const uint32_t* __restrict__ perm,
                                                                  const double* __restrict__ w, int64_t n, int64_t nnz,
                                                                  const int64_t* __restrict__ colptr,
                                                                  uint32_t* __restrict__ rows,
                                                                  double* __restrict__ vals) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const int64_t a = colptr[j], b = colptr[j + 1];
    double m = 0.0;
    for (int64_t t = a; t < b; ++t) {
        const int64_t src = perm[t];
        if (src < nnz && w[src] > m) m = w[src];
    }
    if (b - a <= 1) m = 1.0;  // the loop alone
    double s = 0.0;
    for (int64_t t = a; t < b; ++t) {
        const int64_t src = perm[t];
        s = s + (src < nnz ? w[src] : m);
    }
    for (int64_t t = a; t < b; ++t) {
        const int64_t src = perm[t];
        rows[t] = (uint32_t)(skeys[t] & 0xFFFFFFFFu);
        vals[t] = (src < nnz ? w[src] : m) / s;
    }
}

// ---- the general path ------------------------------------------------------------------

// ec[e] = candidates slot e emits (the length of the column its row names); ec[E] = 0
__global__ __launch_bounds__(kThreads) void mcl_count_kernel(Mat T, int64_t n, int64_t E, int64_t* __restrict__ ec) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e > E) return;
    int64_t c = 0;
    if (e < E) {
        bool valid;
        mat_column(T, n, e, &valid);
        if (valid) c = mat_size(T, T.rows[e]);
    }
    ec[e] = c;
}

// cc[j] = candidates of the columns before j (j <= n)
__global__ __launch_bounds__(kThreads) void mcl_colcand_kernel(Mat T, int64_t n, const int64_t* __restrict__ eoff,
                                                               int64_t* __restrict__ cc) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j <= n) cc[j] = eoff[mat_begin(T, j)];
}

// slots [e0, e1) of a batch write their candidates at eoff[e] - base: column order, then ascending k, then row
__global__ __launch_bounds__(kThreads) void mcl_emit_kernel(Mat T, int64_t n, int64_t e0, int64_t e1,
                                                            const int64_t* __restrict__ eoff, int64_t base,
                                                            uint64_t* __restrict__ keys, double* __restrict__ prod) {
    const int64_t e = e0 + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= e1) return;
    bool valid;
    const int64_t j = mat_column(T, n, e, &valid);
    if (!valid) return;
    const int64_t k = T.rows[e];
    const double tkj = T.vals[e];
    const int64_t kb = mat_begin(T, k), ks = mat_size(T, k);
    const int64_t pos = eoff[e] - base;
    for (int64_t f = 0; f < ks; ++f) {
        keys[pos + f] = (uint64_t)j << 32 | (uint64_t)T.rows[kb + f];
        prod[pos + f] = T.vals[kb + f] * tkj;
    }
}

// the head of each run of equal keys sums its run left to right from +0.0 (ascending k: the sort is stable)
__global__ __launch_bounds__(kThreads) void mcl_runsum_kernel(const uint64_t* __restrict__ skeys,
                                                              const uint32_t* __restrict__ perm,
                                                              const double* __restrict__ prod, int64_t cnt,
                                                              double* __restrict__ xs) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= cnt) return;
    const uint64_t key = skeys[t];
    if (t > 0 && skeys[t - 1] == key) return;
    double s = 0.0;
    for (int64_t u = t; u < cnt && skeys[u] == key; ++u) s = s + prod[perm[u]];
    xs[t] = s;
}

struct IterParams {
    int R;
    double cutoff, inflation;
};

// columns [j0, j1) of a batch: select, prune, normalise, inflate, chaos
__global__ __launch_bounds__(kThreads) void mcl_select_kernel(const uint64_t* __restrict__ skeys,
                                                              const double* __restrict__ xs,
                                                              const int64_t* __restrict__ cc, int64_t base, int64_t j0,
                                                              int64_t j1, IterParams P, uint32_t* __restrict__ orows,
                                                              double* __restrict__ ovals, int32_t* __restrict__ olen,
                                                              unsigned long long* __restrict__ word) {
    const int64_t j = j0 + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= j1) return;
    const int64_t a = cc[j] - base, b = cc[j + 1] - base;
    double bx[kMclRMax];
    uint32_t bi[kMclRMax];
    int nb = 0;
    // the first R heads under (X descending, i ascending); heads arrive by ascending i
    for (int64_t t = a; t < b; ++t) {
        if (t > a && skeys[t - 1] == skeys[t]) continue;
        const double x = xs[t];
        const uint32_t i = (uint32_t)(skeys[t] & 0xFFFFFFFFu);
        int p = nb;
        while (p > 0 && bx[p - 1] < x) --p;  // behind every entry with X >= x
        if (p >= P.R) continue;
        const int last = nb < P.R ? nb : P.R - 1;
        for (int q = last; q > p; --q) {
            bx[q] = bx[q - 1];
            bi[q] = bi[q - 1];
        }
        bx[p] = x;
        bi[p] = i;
        if (nb < P.R) ++nb;
    }
    // keep the first; of the others those with X >= cutoff
    int nk = 1;
    for (int q = 1; q < nb; ++q)
        if (bx[q] >= P.cutoff) {
            bx[nk] = bx[q];
            bi[nk] = bi[q];
            ++nk;
        }
    // by row ascending
    for (int q = 1; q < nk; ++q) {
        const double x = bx[q];
        const uint32_t i = bi[q];
        int p = q;
        while (p > 0 && bi[p - 1] > i) {
            bx[p] = bx[p - 1];
            bi[p] = bi[p - 1];
            --p;
        }
        bx[p] = x;
        bi[p] = i;
    }
    double s = 0.0;
    for (int q = 0; q < nk; ++q) s = s + bx[q];
    double s2 = 0.0;
    for (int q = 0; q < nk; ++q) {
        const double x = bx[q] / s;
        bx[q] = mcl_inflate(x, P.inflation);
        s2 = s2 + bx[q];
    }
    double mx = 0.0, sq = 0.0;
    const int64_t o = j * P.R;
    for (int q = 0; q < nk; ++q) {
        const double z = bx[q] / s2;
        orows[o + q] = bi[q];
        ovals[o + q] = z;
        mx = z > mx ? z : mx;
        sq = sq + z * z;
    }
    olen[j] = nk;
    atomicMax(word, chaos_image(mx - sq));
}

// ---- the fused path --------------------------------------------------------------------

// RR x RR candidates per column, one per lane; R <= RR is the resource (the padded stride)
template <int RR>
__global__ __launch_bounds__(kMclBlock) void mcl_fused_kernel(int64_t n, IterParams P,
                                                              const uint32_t* __restrict__ irows,
                                                              const double* __restrict__ ivals,
                                                              const int32_t* __restrict__ ilen,
                                                              uint32_t* __restrict__ orows,
                                                              double* __restrict__ ovals, int32_t* __restrict__ olen,
                                                              const unsigned long long* __restrict__ prev, double eps,
                                                              unsigned long long* __restrict__ word) {
    constexpr int G = RR * RR;
    constexpr int kCols = kMclBlock / G;
    if (prev) {  // the iteration before this one converged, or did not run: nothing to do
        const unsigned long long p = *prev;
        if (p == 0 || chaos_value(p) < eps) return;
    }
    __shared__ uint64_t skey[kMclBlock];
    __shared__ double sprod[kMclBlock];
    __shared__ double sx[kMclBlock];
    __shared__ uint32_t srow[kMclBlock];
    __shared__ double cx[kCols * RR];
    __shared__ uint32_t ci[kCols * RR];
    __shared__ unsigned long long sch[kCols];

    const int tid = threadIdx.x;
    const int g = tid / G, l = tid % G, gb = g * G;
    const int64_t j = (int64_t)blockIdx.x * kCols + g;
    const bool active = j < n;
    const int R = P.R;
    const int a = l / RR, b = l % RR;

    // one candidate per lane: entry a of column j times entry b of the column it names
    bool valid = false;
    uint32_t i = kNoRow;
    double p = 0.0;
    if (active && a < ilen[j]) {
        const int64_t k = irows[j * R + a];
        if (b < ilen[k]) {
            valid = true;
            i = irows[k * R + b];
            p = ivals[k * R + b] * ivals[j * R + a];
        }
    }
    // rank by (row, lane): the lane order is the k order, columns being ascending by row
    const uint64_t key = (uint64_t)i << 6 | (uint64_t)l;
    skey[tid] = key;
    __syncthreads();
    int rank = 0;
#pragma unroll 8
    for (int m = 0; m < G; ++m) rank += skey[gb + m] < key ? 1 : 0;
    srow[gb + rank] = valid ? i : kNoRow;
    sprod[gb + rank] = p;
    __syncthreads();
    // lane l now stands at sorted position l; a run's head sums it left to right from +0.0
    const uint32_t row = srow[tid];
    const bool head = row != kNoRow && (l == 0 || srow[tid - 1] != row);
    double X = -1.0;
    if (head) {
        X = 0.0;
        for (int u = l; u < G && srow[gb + u] == row; ++u) X = X + sprod[gb + u];
    }
    sx[tid] = X;  // -1: no head (a head's X is never negative)
    __syncthreads();
    // the head's place under (X descending, row ascending)
    int hrank = 0;
#pragma unroll 8
    for (int m = 0; m < G; ++m) {
        const double xm = sx[gb + m];
        hrank += (xm >= 0.0 && (xm > X || (xm == X && srow[gb + m] < row))) ? 1 : 0;
    }
    const bool kept = head && (hrank == 0 || (hrank < R && X >= P.cutoff));
    const unsigned long long wave_mask = __ballot(kept);
    const int shift = (tid & 63) / G * G;  // 0 for a group of 64 lanes
    const unsigned long long gmask = G == 64 ? wave_mask : (wave_mask >> shift) & ((1ull << (G & 63)) - 1ull);
    const int slot = __popcll(gmask & ((1ull << l) - 1ull));
    const int nk = __popcll(gmask);
    if (kept) {  // sorted positions are row ascending: so are the slots
        cx[g * RR + slot] = X;
        ci[g * RR + slot] = row;
    }
    __syncthreads();
    double s = 0.0;
    for (int q = 0; q < nk; ++q) s = s + cx[g * RR + q];
    double y = 0.0;
    if (l < nk) y = mcl_inflate(cx[g * RR + l] / s, P.inflation);
    __syncthreads();
    if (l < nk) cx[g * RR + l] = y;
    __syncthreads();
    double s2 = 0.0;
    for (int q = 0; q < nk; ++q) s2 = s2 + cx[g * RR + q];
    const double z = y / s2;
    __syncthreads();
    if (l < nk) {
        cx[g * RR + l] = z;
        orows[j * R + l] = ci[g * RR + l];
        ovals[j * R + l] = z;
    }
    __syncthreads();
    if (l == 0) {
        unsigned long long image = 0;  // below every column's
        if (active) {
            double mx = 0.0, sq = 0.0;
            for (int q = 0; q < nk; ++q) {
                const double zq = cx[g * RR + q];
                mx = zq > mx ? zq : mx;
                sq = sq + zq * zq;
            }
            olen[j] = nk;
            image = chaos_image(mx - sq);
        }
        sch[g] = image;
    }
    __syncthreads();
    // one atomic per block: a column each on one word serialises (0.5 ms per iteration at 200,000 columns)
    if (tid == 0) {
        unsigned long long m = 0;
        for (int c = 0; c < kCols; ++c) m = sch[c] > m ? sch[c] : m;
        atomicMax(word, m);
    }
}

// padded -> CSC
__global__ __launch_bounds__(kThreads) void mcl_compact_kernel(const uint32_t* __restrict__ prows,
                                                               const double* __restrict__ pvals,
                                                               const int32_t* __restrict__ len, int64_t n, int R,
                                                               const int64_t* __restrict__ colptr,
                                                               uint32_t* __restrict__ rows, double* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n * R) return;
    const int64_t j = e / R, s = e - j * R;
    if (s >= len[j]) return;
    rows[colptr[j] + s] = prows[e];
    vals[colptr[j] + s] = pvals[e];
}

unsigned blocks_of(int64_t count) { return (unsigned)std::max<int64_t>(1, ceil_div(count, kThreads)); }

int key_bits_for(int64_t n) {
    int bits = 1;
    while ((int64_t(1) << bits) <= n) ++bits;
    return 32 + bits;
}

struct Padded {
    DevArray<uint32_t> rows;
    DevArray<double> vals;
    DevArray<uint32_t> len;  // int32 values; n + 1 words, the last one 0 (the scan's total)
    int32_t* len_i() { return reinterpret_cast<int32_t*>(len.ptr); }
};

// One iteration on the general path: T (E slots; begin_of(j) = the first slot of column j, on the host) -> out.
template <typename BeginOf>
int general_iteration(karma_ctx* ctx, const Mat& T, int64_t n, int64_t E, BeginOf begin_of, const IterParams& P,
                      int64_t cand_cap, Padded& out, unsigned long long* word_d, double* chaos) {
    DevArray<int64_t> ec, eoff, cc;
    KARMA_TRY(ec.alloc(ctx, E + 1));
    KARMA_TRY(eoff.alloc(ctx, E + 1));
    KARMA_TRY(cc.alloc(ctx, n + 1));
    KARMA_LAUNCH(ctx, "mcl_expand", mcl_count_kernel, blocks_of(E + 1), kThreads, 0, T, n, E, ec.ptr);
    KARMA_TRY(scan_excl_i64(ctx, ec.ptr, eoff.ptr, E + 1));
    KARMA_LAUNCH(ctx, "mcl_expand", mcl_colcand_kernel, blocks_of(n + 1), kThreads, 0, T, n, eoff.ptr, cc.ptr);
    std::vector<int64_t> cc_h((size_t)n + 1);
    KARMA_HIP(hipMemcpyAsync(cc_h.data(), cc.ptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipMemsetAsync(word_d, 0, 8, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));

    int64_t eff = 0;
    const std::vector<int64_t> bounds = mcl_batches(cc_h.data(), n, cand_cap, &eff);
    KARMA_CHECK(eff <= kMclMaxSort, KARMA_ERR_ARG, "%s", mcl_arg_message(kMclArgsWide));
    int64_t widest = 1;
    for (size_t t = 0; t + 1 < bounds.size(); ++t)
        widest = std::max(widest, cc_h[(size_t)bounds[t + 1]] - cc_h[(size_t)bounds[t]]);
    DevArray<uint64_t> keys, skeys;
    DevArray<double> prod, xs;
    DevArray<uint32_t> perm;
    KARMA_TRY(keys.alloc(ctx, widest));
    KARMA_TRY(skeys.alloc(ctx, widest));
    KARMA_TRY(prod.alloc(ctx, widest));
    KARMA_TRY(xs.alloc(ctx, widest));
    KARMA_TRY(perm.alloc(ctx, widest));
    const int bits = key_bits_for(n);
    for (size_t t = 0; t + 1 < bounds.size(); ++t) {
        const int64_t j0 = bounds[t], j1 = bounds[t + 1];
        const int64_t base = cc_h[(size_t)j0], cnt = cc_h[(size_t)j1] - base;
        const int64_t e0 = begin_of(j0), e1 = begin_of(j1);
        if (cnt <= 0 || e1 <= e0) {
            KARMA_CHECK(false, KARMA_ERR_STATE, "karma_mcl: columns [%lld, %lld) without a candidate", (long long)j0,
                        (long long)j1);
        }
        KARMA_LAUNCH(ctx, "mcl_expand", mcl_emit_kernel, blocks_of(e1 - e0), kThreads, 0, T, n, e0, e1, eoff.ptr, base,
                     keys.ptr, prod.ptr);
        KARMA_TRY(radix_sort_u64(ctx, keys.ptr, nullptr, cnt, bits, skeys.ptr, perm.ptr));
        KARMA_LAUNCH(ctx, "mcl_expand", mcl_runsum_kernel, blocks_of(cnt), kThreads, 0, skeys.ptr, perm.ptr, prod.ptr,
                     cnt, xs.ptr);
        KARMA_LAUNCH(ctx, "mcl_expand", mcl_select_kernel, blocks_of(j1 - j0), kThreads, 0, skeys.ptr, xs.ptr, cc.ptr,
                     base, j0, j1, P, out.rows.ptr, out.vals.ptr, out.len_i(), word_d);
    }
    unsigned long long word = 0;
    KARMA_HIP(hipMemcpyAsync(&word, word_d, 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    KARMA_CHECK(word != 0, KARMA_ERR_STATE, "karma_mcl: an iteration wrote no chaos");
    *chaos = chaos_value(word);
    return KARMA_OK;
}

int launch_fused(karma_ctx* ctx, int64_t n, const IterParams& P, Padded& in, Padded& out,
                 const unsigned long long* prev, double eps, unsigned long long* word) {
    if (P.R <= 4) {
        KARMA_LAUNCH(ctx, "mcl_iter", mcl_fused_kernel<4>, (unsigned)ceil_div(n, kMclBlock / kMclLanesSmall), kMclBlock,
                     0, n, P, in.rows.ptr, in.vals.ptr, in.len_i(), out.rows.ptr, out.vals.ptr, out.len_i(), prev, eps,
                     word);
    } else {
        KARMA_LAUNCH(ctx, "mcl_iter", mcl_fused_kernel<8>, (unsigned)ceil_div(n, kMclBlock / kMclLanesLarge), kMclBlock,
                     0, n, P, in.rows.ptr, in.vals.ptr, in.len_i(), out.rows.ptr, out.vals.ptr, out.len_i(), prev, eps,
                     word);
    }
    return KARMA_OK;
}

}  // namespace

namespace karma {

// The whole computation on device arrays; the final matrix lands in the
// caller's device buffers (colptr n + 1, rows / vals n * resource).
int mcl_device(karma_ctx* ctx, int64_t n, int64_t nnz, const int64_t* off, const uint32_t* nbr, const double* w,
               double inflation, int resource, double cutoff, double eps, int max_iter, int flags, int64_t cand_cap,
               int64_t* colptr, uint32_t* rows, double* vals, int32_t* iterations, double* chaos_out) {
    const int R = resource;
    const IterParams P{R, cutoff, inflation};
    const int64_t total = nnz + n;

    // start: validate, keys, sort, duplicates, column offsets, columns
    DevArray<int> flag;
    DevArray<uint64_t> keys, skeys;
    DevArray<uint32_t> perm, rows0;
    DevArray<double> vals0;
    DevArray<int64_t> cp0;
    KARMA_TRY(flag.alloc(ctx, 1));
    KARMA_TRY(keys.alloc(ctx, total));
    KARMA_TRY(skeys.alloc(ctx, total));
    KARMA_TRY(perm.alloc(ctx, total));
    KARMA_TRY(rows0.alloc(ctx, total));
    KARMA_TRY(vals0.alloc(ctx, total));
    KARMA_TRY(cp0.alloc(ctx, n + 1));
    KARMA_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), ctx->stream));
    KARMA_LAUNCH(ctx, "mcl_start", mcl_validate_kernel, blocks_of(std::max(n, nnz)), kThreads, 0, off, nbr, w, n, nnz,
                 flag.ptr);
    KARMA_LAUNCH(ctx, "mcl_start", mcl_start_keys_kernel, blocks_of(total), kThreads, 0, off, nbr, n, nnz, keys.ptr);
    KARMA_TRY(radix_sort_u64(ctx, keys.ptr, nullptr, total, key_bits_for(n), skeys.ptr, perm.ptr));
    KARMA_LAUNCH(ctx, "mcl_start", mcl_dup_kernel, blocks_of(total), kThreads, 0, skeys.ptr, total, n, flag.ptr);
    KARMA_LAUNCH(ctx, "mcl_start", mcl_colptr_kernel, blocks_of(total + 1), kThreads, 0, skeys.ptr, total, n, cp0.ptr);
    int hflag = 0;
    std::vector<int64_t> cp0_h((size_t)n + 1);
    KARMA_HIP(hipMemcpyAsync(&hflag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipMemcpyAsync(cp0_h.data(), cp0.ptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    KARMA_CHECK(hflag == 0, KARMA_ERR_ARG, "%s",
                mcl_arg_message(hflag & kBadOff      ? kMclArgsOff
                                : hflag & kBadNbr    ? kMclArgsNbr
                                : hflag & kBadWeight ? kMclArgsWeight
                                                     : kMclArgsDup));
    // the weights are indexed with the sorted positions only now that the graph has passed
    KARMA_LAUNCH(ctx, "mcl_start", mcl_start_cols_kernel, blocks_of(n), kThreads, 0, skeys.ptr, perm.ptr, w, n, nnz,
                 cp0.ptr, rows0.ptr, vals0.ptr);
    keys.release();

    Padded buf[2];
    for (Padded& b : buf) {
        KARMA_TRY(b.rows.alloc(ctx, (size_t)n * R));
        KARMA_TRY(b.vals.alloc(ctx, (size_t)n * R));
        KARMA_TRY(b.len.alloc(ctx, n + 1));
        KARMA_HIP(hipMemsetAsync(b.len.ptr, 0, (size_t)(n + 1) * 4, ctx->stream));
    }
    DevArray<unsigned long long> words;
    KARMA_TRY(words.alloc(ctx, kMclQueue));

    // iteration 1: the start matrix's columns are as wide as the degrees
    double chaos = 0.0;
    const Mat T0{cp0.ptr, nullptr, R, rows0.ptr, vals0.ptr};
    KARMA_TRY(general_iteration(
        ctx, T0, n, cp0_h[(size_t)n], [&](int64_t j) { return cp0_h[(size_t)j]; }, P, cand_cap, buf[0], words.ptr,
        &chaos));
    int it = 1, cur = 0;
    const bool fused = R <= kMclFusedMaxR && !(flags & KARMA_MCL_GENERAL);
    while (!(chaos < eps) && it < max_iter) {
        if (!fused) {
            const Mat T{nullptr, buf[cur].len_i(), R, buf[cur].rows.ptr, buf[cur].vals.ptr};
            KARMA_TRY(general_iteration(
                ctx, T, n, n * R, [&](int64_t j) { return j * R; }, P, cand_cap, buf[cur ^ 1], words.ptr, &chaos));
            ++it;
            cur ^= 1;
            continue;
        }
        // a launch whose predecessor converged does nothing: queue a few, then read their words
        const int q = std::min(kMclQueue, max_iter - it);
        unsigned long long wh[kMclQueue] = {};
        KARMA_HIP(hipMemsetAsync(words.ptr, 0, sizeof(wh), ctx->stream));
        for (int s = 0; s < q; ++s)
            KARMA_TRY(launch_fused(ctx, n, P, buf[(cur + s) & 1], buf[(cur + s + 1) & 1],
                                   s ? words.ptr + (s - 1) : nullptr, eps, words.ptr + s));
        KARMA_HIP(hipMemcpyAsync(wh, words.ptr, sizeof(wh), hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        for (int s = 0; s < q; ++s) {
            KARMA_CHECK(wh[s] != 0, KARMA_ERR_STATE, "karma_mcl: an iteration wrote no chaos");
            chaos = chaos_value(wh[s]);
            ++it;
            cur ^= 1;
            if (chaos < eps) break;
        }
    }

    // padded -> CSC
    Padded& fin = buf[cur];
    KARMA_TRY(scan_excl_u32(ctx, fin.len.ptr, colptr, n + 1));
    KARMA_LAUNCH(ctx, "mcl_start", mcl_compact_kernel, blocks_of(n * R), kThreads, 0, fin.rows.ptr, fin.vals.ptr,
                 fin.len_i(), n, R, colptr, rows, vals);
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    *iterations = it;
    *chaos_out = chaos;
    return KARMA_OK;
}

// mcl_device behind the output handling both public entries share
int mcl_run(karma_ctx* ctx, int64_t n, int64_t nnz, const int64_t* off_d, const uint32_t* nbr_d, const double* w_d,
            double inflation, int resource, double cutoff, double eps, int max_iter, int flags, int64_t cand_cap,
            int64_t* colptr, uint32_t* rows, double* vals, int32_t* iterations, double* chaos, int out_is_device) {
    try {
        if (out_is_device)
            return mcl_device(ctx, n, nnz, off_d, nbr_d, w_d, inflation, resource, cutoff, eps, max_iter, flags,
                              cand_cap, colptr, rows, vals, iterations, chaos);
        DevArray<int64_t> cp;
        DevArray<uint32_t> r;
        DevArray<double> v;
        KARMA_TRY(cp.alloc(ctx, n + 1));
        KARMA_TRY(r.alloc(ctx, (size_t)n * resource));
        KARMA_TRY(v.alloc(ctx, (size_t)n * resource));
        KARMA_TRY(mcl_device(ctx, n, nnz, off_d, nbr_d, w_d, inflation, resource, cutoff, eps, max_iter, flags, cand_cap,
                             cp.ptr, r.ptr, v.ptr, iterations, chaos));
        KARMA_HIP(hipMemcpyAsync(colptr, cp.ptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        const int64_t count = colptr[n];
        KARMA_CHECK(count >= n && count <= n * resource, KARMA_ERR_STATE, "karma_mcl: %lld entries in %lld columns",
                    (long long)count, (long long)n);
        KARMA_HIP(hipMemcpyAsync(rows, r.ptr, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipMemcpyAsync(vals, v.ptr, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        return KARMA_OK;
    } catch (const std::bad_alloc&) {
        KARMA_CHECK(false, KARMA_ERR_OOM, "karma_mcl: out of host memory for %lld columns", (long long)n);
    }
    return KARMA_OK;
}

}  // namespace karma

extern "C" {

int karma_mcl_tile(int* v, int n) {
    KARMA_CHECK(v && n >= 0, KARMA_ERR_ARG, "karma_mcl_tile: null out");
    const int64_t all[4] = {kMclTile, kMclLanesSmall, kMclLanesLarge, kMclCandCap};
    for (int t = 0; t < n && t < 4; ++t) v[t] = (int)all[t];
    return KARMA_OK;
}

int karma_mcl(karma_ctx* ctx, int64_t n, const int64_t* off, const uint32_t* nbr, const double* w, int in_is_device,
              double inflation, int resource, double cutoff, double eps, int max_iter, int flags, int64_t cand_cap,
              int64_t* colptr, uint32_t* rows, double* vals, int64_t cap, int32_t* iterations, double* chaos,
              int out_is_device) {
    MclArgError bad = mcl_check_args(n, off, nbr, w, inflation, resource, cutoff, eps, max_iter, flags, cand_cap, colptr,
                                     rows, vals, cap, iterations, chaos);
    if (bad == kMclArgsOk && !in_is_device) {
        try {
            std::vector<int64_t> seen;
            bad = mcl_check_csr(off, nbr, w, n, seen);
        } catch (const std::bad_alloc&) {
            KARMA_CHECK(false, KARMA_ERR_OOM, "karma_mcl: out of host memory for %lld columns", (long long)n);
        }
    }
    KARMA_CHECK(bad == kMclArgsOk, KARMA_ERR_ARG, "%s", mcl_arg_message(bad));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_mcl: null context");
    KARMA_TRY(ctx_begin(ctx));

    int64_t ends[2] = {0, 0};  // off[0], off[n]
    if (in_is_device) {
        KARMA_HIP(hipMemcpyAsync(&ends[0], off, 8, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipMemcpyAsync(&ends[1], off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        bad = mcl_check_nnz(ends[0], ends[1], nbr, w);
        KARMA_CHECK(bad == kMclArgsOk, KARMA_ERR_ARG, "%s", mcl_arg_message(bad));
    } else {
        ends[1] = off[n];
    }
    const int64_t nnz = ends[1];
    DevArray<int64_t> own_off;
    DevArray<uint32_t> own_nbr;
    DevArray<double> own_w;
    const int64_t* off_d = off;
    const uint32_t* nbr_d = nbr;
    const double* w_d = w;
    if (!in_is_device) {
        KARMA_TRY(own_off.alloc(ctx, n + 1));
        KARMA_TRY(own_nbr.alloc(ctx, nnz));
        KARMA_TRY(own_w.alloc(ctx, nnz));
        KARMA_HIP(hipMemcpyAsync(own_off.ptr, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (nnz) {
            KARMA_HIP(hipMemcpyAsync(own_nbr.ptr, nbr, (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream));
            KARMA_HIP(hipMemcpyAsync(own_w.ptr, w, (size_t)nnz * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        off_d = own_off.ptr, nbr_d = own_nbr.ptr, w_d = own_w.ptr;
    }
    return mcl_run(ctx, n, nnz, off_d, nbr_d, w_d, inflation, resource, cutoff, eps, max_iter, flags, cand_cap, colptr,
                   rows, vals, iterations, chaos, out_is_device);
}

}  // extern "C"
