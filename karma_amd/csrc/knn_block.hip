// knn_block.hip — exact k nearest neighbours, one block of candidate rows at a
// time: karma_knn_block folds a block (with a global index base) into per-query
// lists that outlive the call, karma_knn_merge folds two such lists,
// karma_knn_finish turns them into (index, distance).  Kernels
// "profile_knn_block", "profile_knn_merge", "profile_knn_finish".
//
// The distance contract is karma_knn_rows' (include/karma.h, knn.hip): d2 is
// accumulated over the columns in ascending order from +0.0 as acc + t * t,
// each a single round-to-nearest f64 operation; a list is the k smallest
// (d2 bits, index).  The tile is the same too: a block of 16 x 16 threads owns
// kKnnQ query rows, stages kKnnPanel columns of them and of kKnnC candidates
// in LDS, transposed, and every thread accumulates 8 x 8 pairs in registers;
// short panels and rows past the end are staged as zeros.  What differs:
//
//   * queries and candidates are two matrices, and candidate row r has index
//     cand_base + r;
//   * a row's LDS list is loaded from the caller's state (or starts empty) and
//     is written back as (d2 bits u64, index i32), sorted by (bits, index),
//     empty slots (all-ones, INT32_MAX) last; no square root here;
//   * blocks may arrive in any index order, so a candidate enters when the
//     pair (d2, index) is below the list's last (key, index), not when d2
//     alone is below the last key: an equal d2 with a lower index displaces;
//   * with a candidate split S > 1 the grid is ceil(nq / kKnnQ) x S: slice s
//     walks its contiguous share of the candidate tiles from an empty list and
//     writes a partial list to scratch; profile_knn_merge, one wave per row and
//     no atomics, then takes k times the smallest head of the carried list and
//     the S partial ones.
#include "karma_internal.h"
#include "knn_block_args.h"

using namespace karma;

namespace {

constexpr int kQStride = kKnnQ + 2;  // doubles per staged column: 16-byte aligned rows, columns 4 banks apart
constexpr int kCStride = kKnnC + 2;
constexpr int kSlots = kKnnKMax / 16;  // list slots per lane of a row's group
constexpr uint64_t kNoKey = ~uint64_t(0);
constexpr int kNoIdx = 0x7FFFFFFF;
constexpr int kMergeRows = 4;  // rows (waves) per block of profile_knn_merge

static_assert(kKnnThreads == 256 && kKnnQ == 128 && kKnnC == 128, "a 16 x 16 grid of 8 x 8 register tiles");
static_assert(kKnnThreads % kKnnPanel == 0 && kKnnQ % (kKnnThreads / kKnnPanel) == 0, "staging covers the tile");
static_assert(kKnnKMax % 16 == 0, "list slots are dealt to 16 lanes");
static_assert(kKnnKMax <= 64 && kKnnSplitMax + 1 <= 64, "a wave holds a merged list and one head per list");

// compiler and hardware keep a wave's LDS accesses before this point ahead of those after it
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a value the compiler knows nothing about: what is computed from it is not shared with earlier code
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
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

// index of this lane's candidate j of a tile: cbase + 32 (j / 2) + (j % 2).  Unsigned arithmetic: a candidate
// past the block's end (never alive) may lie past INT32_MAX
__device__ __forceinline__ int cand_index(int cbase, int j) {
    return (int)((unsigned)cbase + 32u * (unsigned)(j >> 1) + (unsigned)(j & 1));
}

// The 16 lanes of query row `lr` (local) fold their 8 sums of one candidate
// tile into the row's list.  cvalid: bit j set when candidate j exists.
__device__ __forceinline__ void update_row(const double (&acc)[8], unsigned cvalid, int cbase, int tx, int k,
                                           uint64_t* __restrict__ lkey, int* __restrict__ lidx) {
    uint64_t d[8];
    uint64_t thr = lkey[k - 1];
    int thri = lidx[k - 1];
    unsigned alive = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        d[j] = (uint64_t)__double_as_longlong(acc[j]);
        alive |= (key_less(d[j], cand_index(cbase, j), thr, thri) ? 1u : 0u) << j;
    }
    alive &= cvalid;
    while (__ballot(alive != 0)) {  // uniform over the wave: its four rows step together
        uint64_t bk = kNoKey;
        int bj = 0, bi = kNoIdx;
#pragma unroll
        for (int j = 0; j < 8; ++j)  // ascending j is ascending index: strict < keeps the lowest on a tie
            if (((alive >> j) & 1) && d[j] < bk) bk = d[j], bj = j;
        if (alive) bi = cand_index(cbase, bj);
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
        thri = lidx[k - 1];
        unsigned keep = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) keep |= (key_less(d[j], cand_index(cbase, j), thr, thri) ? 1u : 0u) << j;
        alive &= keep;
    }
}

// Grid (ceil(nq / kKnnQ), S).  in_keys == null: the lists start empty.  Slice s = blockIdx.y reads its lists
// from in_* and writes them to out_* + s * nq * k (S == 1: both are the caller's state).
__global__ __launch_bounds__(kKnnThreads, 2) void profile_knn_block_kernel(
    const double* __restrict__ q, int64_t nq, int64_t ldq, const double* __restrict__ c, int64_t nc, int64_t ldc,
    int64_t m, int64_t cand_base, int k, int S, const uint64_t* in_keys, const int* in_idx, uint64_t* out_keys,
    int* out_idx) {
    __shared__ __attribute__((aligned(16))) double sQ[kKnnPanel * kQStride];
    __shared__ __attribute__((aligned(16))) double sC[kKnnPanel * kCStride];
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lists[];  // kKnnQ x k keys, then kKnnQ x k indices
    uint64_t* const lkeys = reinterpret_cast<uint64_t*>(s_lists);
    int* const lidxs = reinterpret_cast<int*>(s_lists + (size_t)kKnnQ * k * 8);

    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kKnnQ;
    const int64_t tiles = (nc + kKnnC - 1) / kKnnC;
    const int64_t t_lo = knn_slice_begin(tiles, S, (int)blockIdx.y);
    const int64_t t_hi = knn_slice_begin(tiles, S, (int)blockIdx.y + 1);

    // a group's own rows: the carried entries, or empty slots.  The thread's position is taken anew here and
    // at the write-back, so no address of either stays in a register through the tile loop
    {
        const int tid = opaque(threadIdx.x), lx = tid & 15, ly = tid >> 4;
#pragma unroll 1
        for (int qi = 0; qi < 8; ++qi) {
            const int lr = 32 * (qi >> 1) + 2 * ly + (qi & 1);
            const bool carried = in_keys != nullptr && q0 + lr < nq;
            const int64_t o = (q0 + lr) * k;
            for (int s = lx; s < k; s += 16) {
                lkeys[lr * k + s] = carried ? in_keys[o + s] : kNoKey;
                lidxs[lr * k + s] = carried ? in_idx[o + s] : kNoIdx;
            }
        }
    }
    wave_lds_order();

    for (int64_t c0 = t_lo * kKnnC; c0 < t_hi * kKnnC; c0 += kKnnC) {
        double acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

        for (int64_t p0 = 0; p0 < m; p0 += kKnnPanel) {
            __syncthreads();  // the previous panel has been consumed
            stage_panel(q, ldq, q0, nq, p0, m, sQ, kQStride);
            stage_panel(c, ldc, c0, nc, p0, m, sC, kCStride);
            __syncthreads();
#pragma unroll 2
            for (int cc = 0; cc < kKnnPanel; ++cc) {
                double a[8], b[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double2 qa = *reinterpret_cast<const double2*>(&sQ[cc * kQStride + 32 * i + 2 * ty]);
                    const double2 cb = *reinterpret_cast<const double2*>(&sC[cc * kCStride + 32 * i + 2 * tx]);
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

        // an existing candidate's index is at most 2^31 - 2; one past the block's end may wrap (cand_index)
        const int cbase = (int)((unsigned)(cand_base + c0) + 2u * (unsigned)tx);
        unsigned cvalid = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) cvalid |= (c0 + 32 * (j >> 1) + 2 * tx + (j & 1) < nc ? 1u : 0u) << j;
#pragma unroll
        for (int qi = 0; qi < 8; ++qi) {
            const int lr = 32 * (qi >> 1) + 2 * ty + (qi & 1);
            // a row past the end keeps its empty slots (its sums are of staged zeros)
            update_row(acc[qi], q0 + lr < nq ? cvalid : 0u, cbase, tx, k, lkeys + lr * k, lidxs + lr * k);
        }
    }

    wave_lds_order();
    uint64_t* const ok = out_keys + (int64_t)blockIdx.y * nq * k;
    int* const oi = out_idx + (int64_t)blockIdx.y * nq * k;
    const int tid = opaque(threadIdx.x), lx = tid & 15, ly = tid >> 4;
#pragma unroll 1
    for (int qi = 0; qi < 8; ++qi) {
        const int lr = 32 * (qi >> 1) + 2 * ly + (qi & 1);
        if (q0 + lr >= nq) continue;
        const int64_t o = (q0 + lr) * k;
        for (int s = lx; s < k; s += 16) {
            ok[o + s] = lkeys[lr * k + s];
            oi[o + s] = lidxs[lr * k + s];
        }
    }
}

// One wave per row.  Lane 0 walks the row's carried list in keys / idx (when `carried`), lane l in [1, L] list
// l - 1 of lk / li (lists of nq x k, back to back); every lane keeps its list's head.  k rounds: the smallest
// (key, index) of the heads by a butterfly over the wave, kept by lane `round`; the list it came from steps on.
// The row is written once all rounds have read, so the carried list may be overwritten in place.
__global__ __launch_bounds__(64 * kMergeRows) void profile_knn_merge_kernel(uint64_t* keys, int* idx, int carried,
                                                                            const uint64_t* __restrict__ lk,
                                                                            const int* __restrict__ li, int L,
                                                                            int64_t nq, int k) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kMergeRows + (threadIdx.x >> 6);
    if (row >= nq) return;  // the whole wave
    const uint64_t* mk = nullptr;
    const int* mi = nullptr;
    if (lane == 0 && carried) mk = keys + row * k, mi = idx + row * k;
    if (lane >= 1 && lane <= L) mk = lk + ((int64_t)(lane - 1) * nq + row) * k, mi = li + ((int64_t)(lane - 1) * nq + row) * k;
    int pos = 0;
    uint64_t hk = mk ? mk[0] : kNoKey;
    int hi = mk ? mi[0] : kNoIdx;
    uint64_t rk = kNoKey;
    int ri = kNoIdx;
    for (int r = 0; r < k; ++r) {
        uint64_t bk = hk;
        int bi = hi;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const uint64_t ok = __shfl_xor(bk, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            if (key_less(ok, oi, bk, bi)) bk = ok, bi = oi;
        }
        if (lane == r) rk = bk, ri = bi;
        if (mk && hk == bk && hi == bi) {  // an index is offered once: one list (or exhausted ones, at the end)
            ++pos;
            hk = pos < k ? mk[pos] : kNoKey;
            hi = pos < k ? mi[pos] : kNoIdx;
        }
    }
    if (lane < k) keys[row * k + lane] = rk, idx[row * k + lane] = ri;
}

// (d2 bits, index) -> (index, sqrt(d2)); an empty slot -> (-1, +inf)
__global__ __launch_bounds__(256) void profile_knn_finish_kernel(const uint64_t* __restrict__ keys,
                                                                 const int* __restrict__ idx, int64_t count,
                                                                 int* __restrict__ out_idx,
                                                                 double* __restrict__ out_dist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint64_t kk = keys[i];
    const int ii = idx[i];
    const bool empty = kk == kNoKey && ii == kNoIdx;
    out_idx[i] = empty ? -1 : ii;
    out_dist[i] = empty ? __longlong_as_double(0x7FF0000000000000LL) : __dsqrt_rn(__longlong_as_double((long long)kk));
}

// blocks of profile_knn_block resident on the device at once (the smallest lists: the register-bound residency)
int64_t block_capacity(karma_ctx* ctx) {
    return resident_grid(ctx, reinterpret_cast<const void*>(profile_knn_block_kernel), kKnnThreads,
                         (size_t)kKnnQ * 12, INT64_MAX);
}

// A host array's device twin for the length of a call.
template <typename T>
struct Twin {
    DevArray<T> own;
    T* dev = nullptr;
    T* host = nullptr;
    size_t count = 0;
    // the array itself when it is on the device; else a device block, filled from it when `up`
    int open(karma_ctx* ctx, T* p, size_t n, bool is_device, bool up) {
        count = n;
        if (is_device) {
            dev = p;
            return KARMA_OK;
        }
        host = p;
        KARMA_TRY(own.alloc(ctx, n));
        dev = own.ptr;
        if (up && n) KARMA_HIP(hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return KARMA_OK;
    }
    int down(karma_ctx* ctx) {
        if (host && count)
            KARMA_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return KARMA_OK;
    }
};

int launch_merge(karma_ctx* ctx, uint64_t* keys, int* idx, bool carried, const uint64_t* lk, const int* li, int L,
                 int64_t nq, int k) {
    KARMA_LAUNCH(ctx, "profile_knn_merge", profile_knn_merge_kernel, (unsigned)ceil_div(nq, kMergeRows),
                 64 * kMergeRows, 0, keys, idx, carried ? 1 : 0, lk, li, L, nq, k);
    return KARMA_OK;
}

}  // namespace

extern "C" {

int karma_knn_block(karma_ctx* ctx, const double* q, int64_t nq, int64_t ldq, int q_is_device, const double* c,
                    int64_t nc, int64_t ldc, int c_is_device, int64_t m, int64_t cand_base, int k, uint64_t* keys,
                    int32_t* idx, int state_is_device, int first, int cand_split) {
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_knn_block: null context");
    const KnnBlockArgError bad = knn_block_check_args(q, nq, ldq, c, nc, ldc, m, cand_base, k, keys, idx, cand_split);
    KARMA_CHECK(bad == kKnnBlockOk, KARMA_ERR_ARG, "karma_knn_block: %s", knn_block_arg_message(bad));
    KARMA_TRY(ctx_begin(ctx));
    if (nq == 0 || (nc == 0 && !first)) return KARMA_OK;

    // host matrices are copied up without their last row's padding; nothing of them is read without
    // candidates or columns
    const bool reads = nc > 0 && m > 0;
    Twin<double> tq, tc;
    KARMA_TRY(tq.open(ctx, const_cast<double*>(q), reads ? (size_t)(nq - 1) * ldq + m : 0, q_is_device || !reads, true));
    KARMA_TRY(tc.open(ctx, const_cast<double*>(c), reads ? (size_t)(nc - 1) * ldc + m : 0, c_is_device || !reads, true));
    Twin<uint64_t> tk;
    Twin<int32_t> ti;
    KARMA_TRY(tk.open(ctx, keys, (size_t)nq * k, state_is_device, !first));
    KARMA_TRY(ti.open(ctx, idx, (size_t)nq * k, state_is_device, !first));

    const int S = knn_split_resolve(nq, nc, cand_split, cand_split == 0 ? block_capacity(ctx) : 0);
    // the lists beside the 33 KB of staged panels: past 64 KB in all (k > 20) a launch must be allowed its size
    const size_t lds = (size_t)kKnnQ * k * 12;
    if (lds > 30 * 1024)
        KARMA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(profile_knn_block_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)ceil_div(nq, kKnnQ), (unsigned)S);
    const uint64_t* no_keys = nullptr;
    const int* no_idx = nullptr;
    if (S == 1) {
        KARMA_LAUNCH(ctx, "profile_knn_block", profile_knn_block_kernel, grid, kKnnThreads, lds, tq.dev, nq, ldq,
                     tc.dev, nc, ldc, m, cand_base, k, 1, first ? no_keys : tk.dev, first ? no_idx : ti.dev, tk.dev,
                     ti.dev);
    } else {
        DevArray<uint64_t> pk;
        DevArray<int32_t> pi;
        KARMA_TRY(pk.alloc(ctx, (size_t)S * nq * k));
        KARMA_TRY(pi.alloc(ctx, (size_t)S * nq * k));
        KARMA_LAUNCH(ctx, "profile_knn_block", profile_knn_block_kernel, grid, kKnnThreads, lds, tq.dev, nq, ldq,
                     tc.dev, nc, ldc, m, cand_base, k, S, no_keys, no_idx, pk.ptr, pi.ptr);
        KARMA_TRY(launch_merge(ctx, tk.dev, ti.dev, !first, pk.ptr, pi.ptr, S, nq, k));
    }
    KARMA_TRY(tk.down(ctx));
    KARMA_TRY(ti.down(ctx));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    return KARMA_OK;
}

int karma_knn_merge(karma_ctx* ctx, uint64_t* keys, int32_t* idx, const uint64_t* keys_b, const int32_t* idx_b,
                    int64_t nq, int k, int state_is_device) {
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_knn_merge: null context");
    const KnnBlockArgError bad = knn_lists_check_args(keys, idx, keys_b, idx_b, nq, k);
    KARMA_CHECK(bad == kKnnBlockOk, KARMA_ERR_ARG, "karma_knn_merge: %s", knn_block_arg_message(bad));
    KARMA_TRY(ctx_begin(ctx));
    if (nq == 0) return KARMA_OK;
    Twin<uint64_t> tk, bk;
    Twin<int32_t> ti, bi;
    KARMA_TRY(tk.open(ctx, keys, (size_t)nq * k, state_is_device, true));
    KARMA_TRY(ti.open(ctx, idx, (size_t)nq * k, state_is_device, true));
    KARMA_TRY(bk.open(ctx, const_cast<uint64_t*>(keys_b), (size_t)nq * k, state_is_device, true));
    KARMA_TRY(bi.open(ctx, const_cast<int32_t*>(idx_b), (size_t)nq * k, state_is_device, true));
    KARMA_TRY(launch_merge(ctx, tk.dev, ti.dev, true, bk.dev, bi.dev, 1, nq, k));
    KARMA_TRY(tk.down(ctx));
    KARMA_TRY(ti.down(ctx));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    return KARMA_OK;
}

int karma_knn_finish(karma_ctx* ctx, const uint64_t* keys, const int32_t* idx, int64_t nq, int k,
                     int state_is_device, int32_t* out_idx, double* out_dist, int out_is_device) {
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_knn_finish: null context");
    const KnnBlockArgError bad = knn_lists_check_args(keys, idx, out_dist, out_idx, nq, k);
    KARMA_CHECK(bad == kKnnBlockOk, KARMA_ERR_ARG, "karma_knn_finish: %s", knn_block_arg_message(bad));
    KARMA_TRY(ctx_begin(ctx));
    if (nq == 0) return KARMA_OK;
    const size_t count = (size_t)nq * k;
    Twin<uint64_t> tk;
    Twin<int32_t> ti, oi;
    Twin<double> od;
    KARMA_TRY(tk.open(ctx, const_cast<uint64_t*>(keys), count, state_is_device, true));
    KARMA_TRY(ti.open(ctx, const_cast<int32_t*>(idx), count, state_is_device, true));
    KARMA_TRY(oi.open(ctx, out_idx, count, out_is_device, false));
    KARMA_TRY(od.open(ctx, out_dist, count, out_is_device, false));
    KARMA_LAUNCH(ctx, "profile_knn_finish", profile_knn_finish_kernel, (unsigned)ceil_div((int64_t)count, 256), 256, 0,
                 tk.dev, ti.dev, (int64_t)count, oi.dev, od.dev);
    KARMA_TRY(oi.down(ctx));
    KARMA_TRY(od.down(ctx));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    return KARMA_OK;
}

int karma_knn_block_split(karma_ctx* ctx, int64_t nq, int64_t nc, int cand_split, int* used) {
    KARMA_CHECK(used, KARMA_ERR_ARG, "karma_knn_block_split: null out");
    KARMA_CHECK(nq >= 0 && nc >= 0 && nq < kKnnMaxRows && nc <= kKnnMaxIndex, KARMA_ERR_ARG,
                "karma_knn_block_split: %s", knn_block_arg_message(kKnnBlockShape));
    KARMA_CHECK(cand_split >= 0, KARMA_ERR_ARG, "karma_knn_block_split: %s", knn_block_arg_message(kKnnBlockSplit));
    int64_t capacity = 0;
    if (cand_split == 0) {  // auto asks the device; an explicit split is arithmetic alone
        KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_knn_block_split: null context");
        KARMA_TRY(ctx_begin(ctx));
        capacity = block_capacity(ctx);
    }
    *used = knn_split_resolve(nq, nc, cand_split, capacity);
    return KARMA_OK;
}

}  // extern "C"
