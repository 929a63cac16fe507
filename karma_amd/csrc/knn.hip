// knn.hip — exact k nearest neighbours of rows of a dense f64 matrix (the
// device-resident k-mer profile): karma_knn_rows, kernel "profile_knn".
//
// The contract (include/karma.h): d2(i, j) is accumulated over the columns in
// ascending order from +0.0 as acc = acc + t * t, t = x[i, c] - x[j, c], each a
// single round-to-nearest f64 operation (no contraction); a row's list is the
// k rows with the smallest (d2, j), and dist = sqrt(d2) correctly rounded.
//
// A block owns kKnnQ query rows and walks all candidate rows in ascending
// order, kKnnC at a time.  For each pair of tiles it stages kKnnPanel columns
// of both in LDS, transposed (sQ[column][row], so a thread's operands are
// 16-byte LDS reads), and every thread of the 16 x 16 grid accumulates an
// 8 x 8 tile of pairs in registers: thread (ty, tx) holds query rows
// 32 i + 2 ty + e and candidates 32 j + 2 tx + e (i, j < 4; e < 2), which
// puts the sixteen lanes of a 16-byte read on sixty-four different banks.  A
// pair's sum runs over the columns in order, panel after panel; the 64
// independent pairs of a thread are its instruction-level parallelism.  A
// short last panel and rows past the end are staged as zeros: acc + 0 * 0
// leaves acc (>= +0) as it is, bit for bit.
//
// Each query row keeps its k best (d2 bits, index) in LDS, sorted ascending,
// filled with sentinels (all-ones key) until k rows have been seen.  The
// sixteen lanes that share a query row (one ty) own its list: after a
// candidate tile they compare their 8 sums with the list's last key (strict <:
// candidates arrive in ascending index order, so an equal d2 loses), and
// while any of them still has a smaller one, take the group's smallest
// (d2, index) by a butterfly of shuffles and insert it, every lane shifting
// the slots it holds.  Lists are touched by their owning wave alone, so this
// needs no block barrier.  d2 >= +0 (non-finite inputs are outside the
// contract), so the u64 order of the bits is the order of the values.
#include "karma_internal.h"
#include "knn_args.h"

using namespace karma;

namespace {

constexpr int kQStride = kKnnQ + 2;  // doubles per staged column: 16-byte aligned rows, columns 4 banks apart
constexpr int kCStride = kKnnC + 2;
constexpr int kSlots = kKnnKMax / 16;  // list slots per lane of a row's group
constexpr uint64_t kNoKey = ~uint64_t(0);
constexpr int kNoIdx = 0x7FFFFFFF;

static_assert(kKnnThreads == 256 && kKnnQ == 128 && kKnnC == 128, "a 16 x 16 grid of 8 x 8 register tiles");
static_assert(kKnnThreads % kKnnPanel == 0 && kKnnQ % (kKnnThreads / kKnnPanel) == 0, "staging covers the tile");
static_assert(kKnnKMax % 16 == 0, "list slots are dealt to 16 lanes");

// compiler and hardware keep a wave's LDS accesses before this point ahead of those after it
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool key_less(uint64_t a, int ai, uint64_t b, int bi) {
    return a < b || (a == b && ai < bi);
}

// kKnnPanel columns [p0, p0 + kKnnPanel) of rows [r0, r0 + 128) -> dst[column][row]; zeros past n_rows or m
__device__ __forceinline__ void stage_panel(const double* __restrict__ x, int64_t ld, int64_t r0, int64_t n_rows,
                                            int64_t p0, int64_t m, double* __restrict__ dst, int stride) {
    constexpr int kRowsPer = kKnnThreads / kKnnPanel;
    const int col = threadIdx.x % kKnnPanel, row0 = threadIdx.x / kKnnPanel;
    const bool col_ok = p0 + col < m;
    double v[kKnnQ / kRowsPer];
#pragma unroll
    for (int j = 0; j < kKnnQ / kRowsPer; ++j) {
        const int64_t r = r0 + row0 + j * kRowsPer;
        v[j] = (col_ok && r < n_rows) ? x[r * ld + p0 + col] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kKnnQ / kRowsPer; ++j) dst[col * stride + row0 + j * kRowsPer] = v[j];
}

// The 16 lanes of query row `lr` (local) fold their 8 sums of one candidate
// tile into the row's list.  cbase: index of this lane's candidate 0; cand j
// is cbase + 32 (j / 2) + (j % 2); cvalid: bit j set when candidate j exists.
__device__ __forceinline__ void update_row(const double (&acc)[8], unsigned cvalid, int cbase, int tx, int k,
                                           uint64_t* __restrict__ lkey, int* __restrict__ lidx) {
    uint64_t d[8];
    uint64_t thr = lkey[k - 1];
    unsigned alive = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        d[j] = (uint64_t)__double_as_longlong(acc[j]);
        alive |= (d[j] < thr ? 1u : 0u) << j;
    }
    alive &= cvalid;
    while (__ballot(alive != 0)) {  // uniform over the wave: its four rows step together
        uint64_t bk = kNoKey;
        int bj = 0, bi = kNoIdx;
#pragma unroll
        for (int j = 0; j < 8; ++j)  // ascending j is ascending index: strict < keeps the lowest on a tie
            if (((alive >> j) & 1) && d[j] < bk) bk = d[j], bj = j;
        if (alive) bi = cbase + 32 * (bj >> 1) + (bj & 1);
        const int mine = bi;
#pragma unroll
        for (int s = 8; s > 0; s >>= 1) {
            const uint64_t ok = __shfl_xor(bk, s, 16);
            const int oi = __shfl_xor(bi, s, 16);
            if (key_less(ok, oi, bk, bi)) bk = ok, bi = oi;
        }
        const bool any = bi != kNoIdx;  // uniform over the row's 16 lanes
        if (any && mine == bi) alive &= ~(1u << bj);
        // slot s takes: itself if below the new entry, the new entry if its left neighbour is below, else that neighbour
        uint64_t nk[kSlots];
        int ni[kSlots];
#pragma unroll
        for (int u = 0; u < kSlots; ++u) {
            const int s = tx + 16 * u;
            nk[u] = kNoKey, ni[u] = kNoIdx;
            if (any && s < k) {
                const uint64_t ck = lkey[s];
                const int ci = lidx[s];
                const uint64_t pk = s ? lkey[s - 1] : 0;
                const int pi = s ? lidx[s - 1] : -1;
                if (key_less(ck, ci, bk, bi)) nk[u] = ck, ni[u] = ci;
                else if (key_less(pk, pi, bk, bi)) nk[u] = bk, ni[u] = bi;
                else nk[u] = pk, ni[u] = pi;
            }
        }
        wave_lds_order();  // every lane has read before any lane writes
#pragma unroll
        for (int u = 0; u < kSlots; ++u) {
            const int s = tx + 16 * u;
            if (any && s < k) lkey[s] = nk[u], lidx[s] = ni[u];
        }
        wave_lds_order();
        thr = lkey[k - 1];
        unsigned keep = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) keep |= (d[j] < thr ? 1u : 0u) << j;
        alive &= keep;
    }
}

__global__ __launch_bounds__(kKnnThreads, 2) void profile_knn_kernel(const double* __restrict__ x, int64_t n,
                                                                     int64_t m, int64_t ld, int64_t row_lo,
                                                                     int64_t row_hi, int k, int* __restrict__ idx,
                                                                     double* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) double sQ[kKnnPanel * kQStride];
    __shared__ __attribute__((aligned(16))) double sC[kKnnPanel * kCStride];
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lists[];  // kKnnQ x k keys, then kKnnQ x k indices
    uint64_t* const lkeys = reinterpret_cast<uint64_t*>(s_lists);
    int* const lidxs = reinterpret_cast<int*>(s_lists + (size_t)kKnnQ * k * 8);

    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t q0 = row_lo + (int64_t)blockIdx.x * kKnnQ;

    // a group's own rows: sentinels until k candidates have come by
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) {
        const int lr = 32 * (qi >> 1) + 2 * ty + (qi & 1);
        for (int s = tx; s < k; s += 16) lkeys[lr * k + s] = kNoKey, lidxs[lr * k + s] = kNoIdx;
    }
    wave_lds_order();

    for (int64_t c0 = 0; c0 < n; c0 += kKnnC) {
        double acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

        for (int64_t p0 = 0; p0 < m; p0 += kKnnPanel) {
            __syncthreads();  // the previous panel has been consumed
            stage_panel(x, ld, q0, row_hi, p0, m, sQ, kQStride);
            stage_panel(x, ld, c0, n, p0, m, sC, kCStride);
            __syncthreads();
#pragma unroll 2
            for (int c = 0; c < kKnnPanel; ++c) {
                double a[8], b[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double2 qa = *reinterpret_cast<const double2*>(&sQ[c * kQStride + 32 * i + 2 * ty]);
                    const double2 cb = *reinterpret_cast<const double2*>(&sC[c * kCStride + 32 * i + 2 * tx]);
                    a[2 * i] = qa.x, a[2 * i + 1] = qa.y;
                    b[2 * i] = cb.x, b[2 * i + 1] = cb.y;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const double t = __dsub_rn(a[i], b[j]);
                        acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(t, t));
                    }
            }
        }

        const int cbase = (int)c0 + 2 * tx;
        unsigned cvalid = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) cvalid |= (c0 + 32 * (j >> 1) + 2 * tx + (j & 1) < n ? 1u : 0u) << j;
#pragma unroll
        for (int qi = 0; qi < 8; ++qi) {
            const int lr = 32 * (qi >> 1) + 2 * ty + (qi & 1);
            // a row past the range keeps its sentinels (its sums are of staged zeros)
            update_row(acc[qi], q0 + lr < row_hi ? cvalid : 0u, cbase, tx, k, lkeys + lr * k, lidxs + lr * k);
        }
    }

    wave_lds_order();
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) {
        const int lr = 32 * (qi >> 1) + 2 * ty + (qi & 1);
        if (q0 + lr >= row_hi) continue;
        const int64_t o = (q0 + lr - row_lo) * k;
        for (int s = tx; s < k; s += 16) {
            idx[o + s] = lidxs[lr * k + s];
            dist[o + s] = __dsqrt_rn(__longlong_as_double((long long)lkeys[lr * k + s]));
        }
    }
}

}  // namespace

extern "C" {

int karma_knn_tile(int* query_rows, int* cand_rows, int* col_panel, int* k_max) {
    KARMA_CHECK(query_rows && cand_rows && col_panel && k_max, KARMA_ERR_ARG, "karma_knn_tile: null out");
    *query_rows = kKnnQ;
    *cand_rows = kKnnC;
    *col_panel = kKnnPanel;
    *k_max = kKnnKMax;
    return KARMA_OK;
}

int karma_knn_rows(karma_ctx* ctx, const double* x, int64_t n, int64_t m, int64_t ld, int x_is_device,
                   int64_t row_lo, int64_t row_hi, int k, int32_t* idx, double* dist, int out_is_device) {
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_knn_rows: null context");
    const KnnArgError bad = knn_check_args(x, n, m, ld, row_lo, row_hi, k, idx, dist);
    KARMA_CHECK(bad == kKnnArgsOk, KARMA_ERR_ARG, "%s", knn_arg_message(bad));
    KARMA_TRY(ctx_begin(ctx));
    const int64_t rows = row_hi - row_lo;
    if (n == 0 || rows == 0) return KARMA_OK;

    // a host matrix is copied up whole (every row is a candidate), without its last row's padding
    DevArray<double> own;
    DevArray<int32_t> oidx;
    DevArray<double> odist;
    const double* xd = x;
    if (!x_is_device && m > 0) {
        const size_t count = (size_t)(n - 1) * ld + m;
        KARMA_TRY(own.alloc(ctx, count));
        KARMA_HIP(hipMemcpyAsync(own.ptr, x, count * 8, hipMemcpyHostToDevice, ctx->stream));
        xd = own.ptr;
    }
    int32_t* di = idx;
    double* dd = dist;
    if (!out_is_device) {
        KARMA_TRY(oidx.alloc(ctx, (size_t)rows * k));
        KARMA_TRY(odist.alloc(ctx, (size_t)rows * k));
        di = oidx.ptr, dd = odist.ptr;
    }
    // the lists beside the 33 KB of staged panels: past 64 KB in all (k > 20) a launch must be allowed its size
    const size_t lds = (size_t)kKnnQ * k * 12;
    if (lds > 30 * 1024)
        KARMA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(profile_knn_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    KARMA_LAUNCH(ctx, "profile_knn", profile_knn_kernel, (unsigned)ceil_div(rows, kKnnQ), kKnnThreads, lds, xd, n, m,
                 ld, row_lo, row_hi, k, di, dd);
    if (!out_is_device) {
        KARMA_HIP(hipMemcpyAsync(idx, di, (size_t)rows * k * 4, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipMemcpyAsync(dist, dd, (size_t)rows * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    return KARMA_OK;
}

}  // extern "C"
