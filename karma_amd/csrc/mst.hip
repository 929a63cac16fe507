// mst.hip — the exact minimum spanning tree of the mutual-reachability graph of
// the rows of a dense f64 matrix (HDBSCAN's expensive half): karma_mreach_mst.
// Kernels "mst_core", "mst_nearest", "mst_reduce", "mst_hook".
//
// The contract (include/karma.h): d2(i, j) is karma_knn_rows' (columns in
// ascending order from +0.0, acc = acc + t * t, single round-to-nearest f64
// operations); core2(i) is the min_samples-th smallest (d2(i, j), j), row i
// counted; mr2(i, j) = max(d2(i, j), core2(i), core2(j)); the tree is the one
// minimum spanning tree under the strict total order of (mr2 bits, lo, hi).
// Every value is >= +0, so u64 bit patterns order as the values do.
//
// core2 is the last key of the blockwise neighbour lists (karma_knn_block with
// k = min_samples: the unrounded d2 bits).  The tree is built in Boruvka rounds:
//
//   mst_nearest  karma_knn_rows' tile (a block of 16 x 16 threads owns kKnnQ
//                query rows, stages kKnnPanel columns of them and of kKnnC
//                candidates in LDS, every thread accumulates 8 x 8 pairs), with
//                the candidates' component ids and core2 staged beside them.
//                A row keeps the smallest (mr2, j) over the rows j of another
//                component: for a fixed i the smallest j among equal mr2 is
//                also the smallest (lo, hi).  The candidate tiles are dealt to
//                S slices (grid.y), each writing its partial answer.  A tile
//                whose rows and the block's rows all share one component (by
//                the per-tile smallest and largest ids) is skipped: it holds no
//                candidate at all.
//   mst_reduce   pass 0 folds a row's S partial answers and takes the smallest
//                mr2 per component with a 64-bit atomicMin; pass 1 takes the
//                smallest lo << 32 | hi among the rows that hold that mr2.
//   mst_hook     a component hooks to the one its edge leads to.  Under a
//                strict total order the only cycles are two components picking
//                the same edge: the lower id stays a root and appends the edge,
//                the other hooks without appending.  Then pointer jumping to
//                the roots, and the rows take their root's id.
//
// The host reads the edge count once per round, and sorts the n - 1 edges by
// their key at the end, so the order in which edges were appended is gone.
#include <algorithm>
#include <new>
#include <numeric>

#include "karma_internal.h"
#include "mst_args.h"

using namespace karma;

namespace {

constexpr int kQStride = kKnnQ + 2;  // doubles per staged column: 16-byte aligned rows, columns 4 banks apart
constexpr int kCStride = kKnnC + 2;
constexpr uint64_t kNoKey = ~uint64_t(0);
constexpr int kNoIdx = 0x7FFFFFFF;
constexpr int kRowThreads = 128;  // per-row kernels: one block per tile of kKnnC rows

static_assert(kKnnThreads == 256 && kKnnQ == 128 && kKnnC == 128, "a 16 x 16 grid of 8 x 8 register tiles");
static_assert(kKnnThreads % kKnnPanel == 0 && kKnnQ % (kKnnThreads / kKnnPanel) == 0, "staging covers the tile");
static_assert(kRowThreads == kKnnC && kKnnQ == kKnnC, "one range per tile serves queries and candidates");

__device__ __forceinline__ bool key_less(uint64_t a, int ai, uint64_t b, int bi) {
    return a < b || (a == b && ai < bi);
}

__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

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

// The smallest and largest component id of a tile's rows (one block of kRowThreads per tile).
__device__ __forceinline__ void tile_range(int id, bool valid, int* __restrict__ tile_lo, int* __restrict__ tile_hi) {
    __shared__ int s_lo, s_hi;
    if (threadIdx.x == 0) s_lo = kNoIdx, s_hi = -1;
    __syncthreads();
    if (valid) {
        atomicMin(&s_lo, id);
        atomicMax(&s_hi, id);
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_lo[blockIdx.x] = s_lo, tile_hi[blockIdx.x] = s_hi;
}

// core2 = a row's last list key; every row starts as its own component
__global__ __launch_bounds__(kRowThreads) void mst_core_kernel(const uint64_t* __restrict__ keys, int64_t n, int k,
                                                               uint64_t* __restrict__ core2, double* __restrict__ core,
                                                               int* __restrict__ comp, int* __restrict__ parent,
                                                               int* __restrict__ tile_lo, int* __restrict__ tile_hi) {
    const int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (i < n) {
        const uint64_t c2 = keys[i * k + (k - 1)];
        core2[i] = c2;
        core[i] = __dsqrt_rn(__longlong_as_double((long long)c2));
        comp[i] = (int)i;
        parent[i] = (int)i;
    }
    tile_range((int)i, i < n, tile_lo, tile_hi);
}

// Grid (ceil(n / kKnnQ), S).  Slice s = blockIdx.y writes, for every row i, the smallest (mr2 bits, j) over the
// rows j of its candidate tiles that lie in another component to out_key / out_j [s * n + i]; (all-ones,
// INT32_MAX) when it has none.
__global__ __launch_bounds__(kKnnThreads, 2) void mst_nearest_kernel(
    const double* __restrict__ x, int64_t n, int64_t m, int64_t ld, const uint64_t* __restrict__ core2,
    const int* __restrict__ comp, const int* __restrict__ tile_lo, const int* __restrict__ tile_hi, int S,
    uint64_t* __restrict__ out_key, int* __restrict__ out_j) {
    __shared__ __attribute__((aligned(16))) double sQ[kKnnPanel * kQStride];
    __shared__ __attribute__((aligned(16))) double sC[kKnnPanel * kCStride];
    __shared__ uint64_t sCore[kKnnC], sQCore[kKnnQ];  // the query rows' values wait here, not in registers
    __shared__ int sComp[kKnnC], sQComp[kKnnQ];

    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kKnnQ;
    const int64_t tiles = (n + kKnnC - 1) / kKnnC;
    const int64_t t_lo = tiles * (int64_t)blockIdx.y / S, t_hi = tiles * ((int64_t)blockIdx.y + 1) / S;
    const int q_lo = tile_lo[blockIdx.x], q_hi = tile_hi[blockIdx.x];

    if (threadIdx.x < kKnnQ) {
        const int64_t r = q0 + threadIdx.x;
        sQCore[threadIdx.x] = r < n ? core2[r] : 0;
        sQComp[threadIdx.x] = r < n ? comp[r] : -1;  // a row past the end takes no candidate
    }
    __syncthreads();
    uint64_t bk[8];
    int bj[8];
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) bk[qi] = kNoKey, bj[qi] = kNoIdx;

    for (int64_t t = t_lo; t < t_hi; ++t) {
        // uniform over the block: nothing here lies in another component
        if (q_lo == q_hi && tile_lo[t] == q_lo && tile_hi[t] == q_lo) continue;
        const int64_t c0 = t * kKnnC;
        __syncthreads();  // the previous tile's ids and core2 have been consumed
        if (threadIdx.x < kKnnC) {
            const int64_t r = c0 + threadIdx.x;
            sCore[threadIdx.x] = r < n ? core2[r] : 0;
            sComp[threadIdx.x] = r < n ? comp[r] : -1;
        }
        __syncthreads();

        double acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

        for (int64_t p0 = 0; p0 < m; p0 += kKnnPanel) {
            __syncthreads();  // the previous panel has been consumed
            stage_panel(x, ld, q0, n, p0, m, sQ, kQStride);
            stage_panel(x, ld, c0, n, p0, m, sC, kCStride);
            __syncthreads();
            // a short last panel stops at column m: the zeros staged past it would add nothing, bit for bit
            const int cols = m - p0 < kKnnPanel ? (int)(m - p0) : kKnnPanel;
#pragma unroll 2
            for (int c = 0; c < cols; ++c) {
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
                        const double t2 = __dsub_rn(a[i], b[j]);
                        acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(t2, t2));
                    }
            }
        }

#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lc = 32 * (j >> 1) + 2 * tx + (j & 1);
            const int ccomp = sComp[lc];  // -1 past the end: such a candidate is never taken
            const uint64_t ccore = sCore[lc];
            const int cj = (int)(c0 + lc);
#pragma unroll
            for (int qi = 0; qi < 8; ++qi) {
                const int lq = 32 * (qi >> 1) + 2 * ty + (qi & 1);
                const int qcomp = sQComp[lq];
                const uint64_t key =
                    max_u64(max_u64((uint64_t)__double_as_longlong(acc[qi][j]), sQCore[lq]), ccore);
                const bool foreign = ccomp >= 0 && qcomp >= 0 && ccomp != qcomp;
                if (foreign && key_less(key, cj, bk[qi], bj[qi])) bk[qi] = key, bj[qi] = cj;
            }
        }
    }

    // the sixteen lanes that share a query row fold their answers
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) {
#pragma unroll
        for (int s = 8; s > 0; s >>= 1) {
            const uint64_t ok = __shfl_xor(bk[qi], s, 16);
            const int oj = __shfl_xor(bj[qi], s, 16);
            if (key_less(ok, oj, bk[qi], bj[qi])) bk[qi] = ok, bj[qi] = oj;
        }
        const int64_t r = q0 + 32 * (qi >> 1) + 2 * ty + (qi & 1);
        if (tx == 0 && r < n) {
            out_key[(int64_t)blockIdx.y * n + r] = bk[qi];
            out_j[(int64_t)blockIdx.y * n + r] = bj[qi];
        }
    }
}

// pass 0: row_key / row_j = the smallest of a row's S partial answers; cmin[component] = the smallest mr2 bits.
// pass 1: cpair[component] = the smallest lo << 32 | hi among its rows whose mr2 is cmin.
__global__ __launch_bounds__(256) void mst_reduce_kernel(int pass, int64_t n, int S,
                                                         const uint64_t* __restrict__ part_key,
                                                         const int* __restrict__ part_j, uint64_t* __restrict__ row_key,
                                                         int* __restrict__ row_j, const int* __restrict__ comp,
                                                         unsigned long long* __restrict__ cmin,
                                                         unsigned long long* __restrict__ cpair) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (pass == 0) {
        uint64_t k = kNoKey;
        int j = kNoIdx;
        for (int s = 0; s < S; ++s) {
            const uint64_t pk = part_key[(int64_t)s * n + i];
            const int pj = part_j[(int64_t)s * n + i];
            if (key_less(pk, pj, k, j)) k = pk, j = pj;
        }
        row_key[i] = k;
        row_j[i] = j;
        if (j != kNoIdx) atomicMin(&cmin[comp[i]], (unsigned long long)k);
    } else {
        const int j = row_j[i];
        if (j == kNoIdx) return;
        const int c = comp[i];
        if (row_key[i] != cmin[c]) return;
        const uint64_t lo = (uint64_t)(i < j ? i : j), hi = (uint64_t)(i < j ? j : i);
        atomicMin(&cpair[c], (unsigned long long)(lo << 32 | hi));
    }
}

// One thread per component id c that has an edge this round (cmin[c] set).
__global__ __launch_bounds__(256) void mst_hook_kernel(int64_t n, const int* __restrict__ comp,
                                                       const unsigned long long* __restrict__ cmin,
                                                       const unsigned long long* __restrict__ cpair,
                                                       int* __restrict__ parent, unsigned* __restrict__ edge_count,
                                                       uint64_t* __restrict__ edge_key,
                                                       uint64_t* __restrict__ edge_pair) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const uint64_t key = cmin[c];
    if (key == kNoKey) return;
    const uint64_t pair = cpair[c];
    const int cl = comp[pair >> 32], ch = comp[pair & 0xFFFFFFFFu];
    const int d = cl == (int)c ? ch : cl;
    const bool mutual = cmin[d] == key && cpair[d] == pair;
    if (mutual && (int)c < d) {
        // stays a root
    } else {
        parent[c] = d;
        if (mutual) return;  // the root of the pair appends the edge
    }
    const unsigned pos = atomicAdd(edge_count, 1u);
    if ((int64_t)pos < n - 1) edge_key[pos] = key, edge_pair[pos] = pair;
}

// One step of pointer jumping, in place: whatever a thread reads of another's entry is one of its ancestors.
__global__ __launch_bounds__(256) void mst_jump_kernel(int64_t n, int* parent) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const int p = __atomic_load_n(&parent[c], __ATOMIC_RELAXED);
    const int g = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (g != p) __atomic_store_n(&parent[c], g, __ATOMIC_RELAXED);
}

// rows take their root's id (parent holds roots by now); the tiles' id ranges for the next round
__global__ __launch_bounds__(kRowThreads) void mst_relabel_kernel(int64_t n, const int* __restrict__ parent,
                                                                  int* __restrict__ comp, int* __restrict__ tile_lo,
                                                                  int* __restrict__ tile_hi) {
    const int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    int id = 0;
    if (i < n) {
        id = parent[comp[i]];
        comp[i] = id;
    }
    tile_range(id, i < n, tile_lo, tile_hi);
}

template <typename T>
int fetch(karma_ctx* ctx, T* host, const T* dev, size_t count) {
    if (count) KARMA_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return KARMA_OK;
}

template <typename T>
int deliver(karma_ctx* ctx, T* out, const T* host, size_t count, bool out_is_device) {
    if (!count) return KARMA_OK;
    if (out_is_device) {
        KARMA_HIP(hipMemcpyAsync(out, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    } else {
        std::copy(host, host + count, out);
    }
    return KARMA_OK;
}

}  // namespace

extern "C" {

int karma_mst_tile(int* query_rows, int* cand_rows, int* col_panel, int* rounds_max) {
    KARMA_CHECK(query_rows && cand_rows && col_panel && rounds_max, KARMA_ERR_ARG, "karma_mst_tile: null out");
    *query_rows = kKnnQ;
    *cand_rows = kKnnC;
    *col_panel = kKnnPanel;
    *rounds_max = mst_rounds_max(kKnnMaxRows - 1);
    return KARMA_OK;
}

int karma_mreach_mst(karma_ctx* ctx, const double* x, int64_t n, int64_t m, int64_t ld, int x_is_device,
                     int min_samples, int32_t* a, int32_t* b, double* w, double* core, int out_is_device) {
    const MstArgError bad = mst_check_args(x, n, m, ld, min_samples, a, b, w, core);
    KARMA_CHECK(bad == kMstArgsOk, KARMA_ERR_ARG, "%s", mst_arg_message(bad));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_mreach_mst: null context");
    KARMA_TRY(ctx_begin(ctx));
    const int k = min_samples;
    const int64_t tiles = ceil_div(n, kKnnC), edges = n - 1;

    // a host matrix is copied up whole (every row is a candidate), without its last row's padding
    DevArray<double> own;
    const double* xd = x;
    if (!x_is_device && m > 0) {
        const size_t count = (size_t)(n - 1) * ld + m;
        KARMA_TRY(own.alloc(ctx, count));
        KARMA_HIP(hipMemcpyAsync(own.ptr, x, count * 8, hipMemcpyHostToDevice, ctx->stream));
        xd = own.ptr;
    }

    DevArray<uint64_t> core2;
    DevArray<double> dcore;
    DevArray<int> comp, parent, tile_lo, tile_hi;
    KARMA_TRY(core2.alloc(ctx, n));
    KARMA_TRY(comp.alloc(ctx, n));
    KARMA_TRY(parent.alloc(ctx, n));
    KARMA_TRY(tile_lo.alloc(ctx, tiles));
    KARMA_TRY(tile_hi.alloc(ctx, tiles));
    double* core_dev = core;
    if (!out_is_device) {
        KARMA_TRY(dcore.alloc(ctx, n));
        core_dev = dcore.ptr;
    }
    {  // the neighbour lists live only until core2 has been taken from them
        DevArray<uint64_t> keys;
        DevArray<int32_t> idx;
        KARMA_TRY(keys.alloc(ctx, (size_t)n * k));
        KARMA_TRY(idx.alloc(ctx, (size_t)n * k));
        KARMA_TRY(karma_knn_block(ctx, xd, n, ld, 1, xd, n, ld, 1, m, 0, k, keys.ptr, idx.ptr, 1, 1, 0));
        KARMA_LAUNCH(ctx, "mst_core", mst_core_kernel, (unsigned)tiles, kRowThreads, 0, keys.ptr, n, k, core2.ptr,
                     core_dev, comp.ptr, parent.ptr, tile_lo.ptr, tile_hi.ptr);
        if (!out_is_device) KARMA_TRY(fetch(ctx, core, core_dev, (size_t)n));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (edges == 0) return KARMA_OK;

    const int S = mst_split(n, resident_grid(ctx, reinterpret_cast<const void*>(mst_nearest_kernel), kKnnThreads, 0,
                                             INT64_MAX));
    DevArray<uint64_t> part_key, row_key, edge_key, edge_pair;
    DevArray<int> part_j, row_j;
    DevArray<unsigned long long> cmin, cpair;
    DevArray<unsigned> edge_count;
    KARMA_TRY(part_key.alloc(ctx, (size_t)S * n));
    KARMA_TRY(part_j.alloc(ctx, (size_t)S * n));
    KARMA_TRY(row_key.alloc(ctx, n));
    KARMA_TRY(row_j.alloc(ctx, n));
    KARMA_TRY(cmin.alloc(ctx, n));
    KARMA_TRY(cpair.alloc(ctx, n));
    KARMA_TRY(edge_key.alloc(ctx, edges));
    KARMA_TRY(edge_pair.alloc(ctx, edges));
    KARMA_TRY(edge_count.alloc(ctx, 1));
    KARMA_HIP(hipMemsetAsync(edge_count.ptr, 0, sizeof(unsigned), ctx->stream));

    const unsigned row_blocks = (unsigned)ceil_div(n, 256);
    const dim3 grid((unsigned)ceil_div(n, kKnnQ), (unsigned)S);
    const int rounds_max = mst_rounds_max(n);
    int64_t found = 0;
    for (int round = 0; found < edges; ++round) {
        KARMA_CHECK(round < rounds_max, KARMA_ERR_STATE, "karma_mreach_mst: %lld of %lld edges after %d rounds",
                    (long long)found, (long long)edges, round);
        KARMA_HIP(hipMemsetAsync(cmin.ptr, 0xFF, (size_t)n * 8, ctx->stream));
        KARMA_HIP(hipMemsetAsync(cpair.ptr, 0xFF, (size_t)n * 8, ctx->stream));
        KARMA_LAUNCH(ctx, "mst_nearest", mst_nearest_kernel, grid, kKnnThreads, 0, xd, n, m, ld, core2.ptr, comp.ptr,
                     tile_lo.ptr, tile_hi.ptr, S, part_key.ptr, part_j.ptr);
        for (int pass = 0; pass < 2; ++pass)
            KARMA_LAUNCH(ctx, "mst_reduce", mst_reduce_kernel, row_blocks, 256, 0, pass, n, S, part_key.ptr,
                         part_j.ptr, row_key.ptr, row_j.ptr, comp.ptr, cmin.ptr, cpair.ptr);
        KARMA_LAUNCH(ctx, "mst_hook", mst_hook_kernel, row_blocks, 256, 0, n, comp.ptr, cmin.ptr, cpair.ptr,
                     parent.ptr, edge_count.ptr, edge_key.ptr, edge_pair.ptr);
        // a round's hooks make chains of at most (components) ids; a jump halves their length
        for (int j = mst_rounds_max(n - found); j > 0; --j)
            KARMA_LAUNCH(ctx, "mst_hook", mst_jump_kernel, row_blocks, 256, 0, n, parent.ptr);
        KARMA_LAUNCH(ctx, "mst_hook", mst_relabel_kernel, (unsigned)tiles, kRowThreads, 0, n, parent.ptr, comp.ptr,
                     tile_lo.ptr, tile_hi.ptr);
        void* pin = nullptr;
        KARMA_TRY(ctx_pinned(ctx, sizeof(unsigned), &pin));
        KARMA_TRY(fetch(ctx, static_cast<unsigned*>(pin), edge_count.ptr, 1));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        const int64_t now = *static_cast<unsigned*>(pin);
        KARMA_CHECK(now > found && now <= edges, KARMA_ERR_STATE,
                    "karma_mreach_mst: round %d went from %lld to %lld of %lld edges", round, (long long)found,
                    (long long)now, (long long)edges);
        found = now;
    }

    // the output order: ascending (mr2 bits, lo, hi)
    try {
        std::vector<uint64_t> hk((size_t)edges), hp((size_t)edges);
        KARMA_TRY(fetch(ctx, hk.data(), edge_key.ptr, (size_t)edges));
        KARMA_TRY(fetch(ctx, hp.data(), edge_pair.ptr, (size_t)edges));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        std::vector<int64_t> order((size_t)edges);
        std::iota(order.begin(), order.end(), int64_t(0));
        std::sort(order.begin(), order.end(),
                  [&](int64_t p, int64_t q) { return hk[p] < hk[q] || (hk[p] == hk[q] && hp[p] < hp[q]); });
        std::vector<int32_t> ha((size_t)edges), hb((size_t)edges);
        std::vector<double> hw((size_t)edges);
        for (int64_t e = 0; e < edges; ++e) {
            const uint64_t key = hk[order[e]], pair = hp[order[e]];
            double d2;
            static_assert(sizeof(d2) == sizeof(key), "f64 bits");
            __builtin_memcpy(&d2, &key, 8);
            ha[e] = (int32_t)(pair >> 32);
            hb[e] = (int32_t)(pair & 0xFFFFFFFFu);
            hw[e] = __builtin_sqrt(d2);  // IEEE: correctly rounded
        }
        KARMA_TRY(deliver(ctx, a, ha.data(), (size_t)edges, out_is_device != 0));
        KARMA_TRY(deliver(ctx, b, hb.data(), (size_t)edges, out_is_device != 0));
        KARMA_TRY(deliver(ctx, w, hw.data(), (size_t)edges, out_is_device != 0));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
    } catch (const std::bad_alloc&) {
        KARMA_CHECK(false, KARMA_ERR_OOM, "karma_mreach_mst: out of host memory for %lld edges", (long long)edges);
    }
    return KARMA_OK;
}

}  // extern "C"
