// umap.hip — UMAP on the device: the fuzzy simplicial set of exact neighbour
// lists (karma_umap_graph) and the layout in gather form (karma_umap_layout).
// Kernels "umap_graph" (rows, sigma, entries, indptr, gather) and
// "umap_layout" (validate, schedule, init, one launch per epoch).
//
// The contract (include/karma.h) defines every output bit; the arithmetic is in
// umap_math.h, shared with the host.  No floating-point atomics anywhere.
//
// The graph.  A thread per row finds rho and the row's sum; the host adds the n
// row sums in row order (the global mean of the floor).  A thread per row then
// bisects sigma and writes the row's k memberships.  A thread per directed
// entry (i -> c) looks i up in row c's list (k entries): with p its own
// membership and q the opposite one (0 where absent) it emits the key
// i << 32 | c with w = (p + q) - p * q, and, where row c does not name i, the
// mirrored key c << 32 | i as well: each unordered pair is emitted exactly once
// per direction, with no atomics and no reverse lists.  Self entries and w == 0
// take the key n << 32, past every row.  One radix sort of the 2 n k keys puts
// the rows in order and each row ascending by column, whatever order the
// threads ran in; indptr is read off the sorted keys' row changes.
//
// The layout.  A thread per vertex walks its CSR row (umap_vertex_epoch): its
// own coordinates are live in registers, everyone else's are read from the
// epoch's start (y_old), and it alone writes y_new[i] and its row's schedule
// words.  One launch per epoch, the two buffers swapped; the host does not wait
// inside the loop.  A hub's row is walked by the one thread that owns it.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "karma_internal.h"
#include "umap_args.h"
#include "umap_math.h"

using namespace karma;

namespace {

constexpr int kEntryThreads = 256;
static_assert(kUmapMaxDim == kUmapDimMax, "the layout kernel is instantiated for every dim the checks let through");

// rho[i], row_sum[i]; *bad set where a list names a row outside [0, n)
__global__ __launch_bounds__(kUmapTile) void umap_rows_kernel(const int32_t* __restrict__ idx,
                                                              const double* __restrict__ dist, int64_t n, int k,
                                                              double* __restrict__ rho, double* __restrict__ row_sum,
                                                              int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * kUmapTile + threadIdx.x;
    if (i >= n) return;
    bool out = false;
    for (int j = 0; j < k; ++j) {
        const int32_t c = idx[i * k + j];
        out |= c < 0 || (int64_t)c >= n;
    }
    if (out) atomicOr(bad, 1);
    umap_row_rho(dist + i * k, k, &rho[i], &row_sum[i]);
}

// sigma[i] and the row's memberships (-1 for a self entry)
__global__ __launch_bounds__(kUmapTile) void umap_sigma_kernel(const int32_t* __restrict__ idx,
                                                               const double* __restrict__ dist, int64_t n, int k,
                                                               const double* __restrict__ rho,
                                                               const double* __restrict__ row_sum, double global_mean,
                                                               double target, double* __restrict__ sigma,
                                                               double* __restrict__ memb) {
    const int64_t i = (int64_t)blockIdx.x * kUmapTile + threadIdx.x;
    if (i >= n) return;
    const double r = rho[i];
    const double s = umap_row_sigma(idx + i * k, dist + i * k, k, i, r, row_sum[i], global_mean, target);
    sigma[i] = s;
    for (int j = 0; j < k; ++j)
        memb[i * k + j] = (int64_t)idx[i * k + j] == i ? -1.0 : umap_membership(dist[i * k + j], r, s);
}

// entry e = i * k + slot -> keys[e] (the entry itself) and keys[E + e] (its mirror, where row c does not name i)
__global__ __launch_bounds__(kEntryThreads) void umap_entries_kernel(const int32_t* __restrict__ idx,
                                                                     const double* __restrict__ memb, int64_t n, int k,
                                                                     uint64_t* __restrict__ keys,
                                                                     double* __restrict__ w_out) {
    const int64_t E = n * k;
    const int64_t e = (int64_t)blockIdx.x * kEntryThreads + threadIdx.x;
    if (e >= E) return;
    const uint64_t none = (uint64_t)n << 32;
    const int64_t i = e / k;
    const int64_t c = idx[e];
    const double p = memb[e];
    uint64_t own = none, mirror = none;
    double w = 0.0;
    if (c != i) {
        double q = 0.0;
        bool named = false;
        for (int j = 0; j < k; ++j)
            if ((int64_t)idx[c * k + j] == i) {
                q = memb[c * k + j];
                named = true;
            }
        w = (p + q) - p * q;
        if (w != 0.0) {
            own = (uint64_t)i << 32 | (uint64_t)c;
            if (!named) mirror = (uint64_t)c << 32 | (uint64_t)i;
        }
    }
    keys[e] = own;
    keys[E + e] = mirror;
    w_out[e] = w;
    w_out[E + e] = w;
}

// sorted keys -> indptr: position t opens every row in (row of t - 1, row of t]; the row n stands past the end
__global__ __launch_bounds__(kEntryThreads) void umap_indptr_kernel(const uint64_t* __restrict__ skeys, int64_t total,
                                                                    int64_t n, int64_t* __restrict__ indptr) {
    const int64_t t = (int64_t)blockIdx.x * kEntryThreads + threadIdx.x;
    if (t > total) return;
    const int64_t cur = t < total ? (int64_t)(skeys[t] >> 32) : n;
    const int64_t prev = t > 0 ? (int64_t)(skeys[t - 1] >> 32) : -1;
    for (int64_t r = prev + 1; r <= cur && r <= n; ++r) indptr[r] = t;
}

__global__ __launch_bounds__(kEntryThreads) void umap_gather_kernel(const uint64_t* __restrict__ skeys,
                                                                    const uint32_t* __restrict__ perm,
                                                                    const double* __restrict__ w_in, int64_t total,
                                                                    int64_t n, int32_t* __restrict__ indices,
                                                                    double* __restrict__ weights) {
    const int64_t t = (int64_t)blockIdx.x * kEntryThreads + threadIdx.x;
    if (t >= total) return;
    const uint64_t key = skeys[t];
    if ((int64_t)(key >> 32) >= n) return;
    indices[t] = (int32_t)(key & 0xFFFFFFFFu);
    weights[t] = w_in[perm[t]];
}

// ---- layout ---------------------------------------------------------------------------

enum : int { kBadIndptr = 1, kBadColumn = 2, kBadWeight = 4 };

// a device graph's contents, checked before anything indexes with them; the largest weight's bits
__global__ __launch_bounds__(kEntryThreads) void umap_validate_kernel(const int64_t* __restrict__ indptr,
                                                                      const int32_t* __restrict__ indices,
                                                                      const double* __restrict__ weights, int64_t n,
                                                                      int64_t nnz, int* __restrict__ bad,
                                                                      unsigned long long* __restrict__ wmax_bits) {
    const int64_t t = (int64_t)blockIdx.x * kEntryThreads + threadIdx.x;
    int flags = 0;
    if (t < n && indptr[t + 1] < indptr[t]) flags |= kBadIndptr;
    if (t == 0 && (indptr[0] != 0 || indptr[n] != nnz)) flags |= kBadIndptr;
    if (t < nnz) {
        const int32_t c = indices[t];
        const double w = weights[t];
        if (c < 0 || (int64_t)c >= n) flags |= kBadColumn;
        if (!(w > 0.0) || w == INFINITY) {
            flags |= kBadWeight;
        } else {
            atomicMax(wmax_bits, (unsigned long long)__double_as_longlong(w));  // w > 0: the bits order as the values
        }
    }
    if (flags) atomicOr(bad, flags);
}

// eps = wmax / w and the first firing epochs; an entry below wmax / n_epochs never fires (eons = +inf)
__global__ __launch_bounds__(kEntryThreads) void umap_schedule_kernel(const double* __restrict__ weights, int64_t nnz,
                                                                      const unsigned long long* __restrict__ wmax_bits,
                                                                      int n_epochs, int R, double* __restrict__ eps,
                                                                      double* __restrict__ eons,
                                                                      double* __restrict__ eonns,
                                                                      uint32_t* __restrict__ t) {
    const int64_t e = (int64_t)blockIdx.x * kEntryThreads + threadIdx.x;
    if (e >= nnz) return;
    const double wmax = __longlong_as_double((long long)*wmax_bits);
    const double w = weights[e];
    const bool active = w >= wmax / (double)n_epochs;
    const double ee = active ? wmax / w : 0.0;
    eps[e] = ee;
    eons[e] = active ? ee : INFINITY;
    eonns[e] = (active && R > 0) ? ee / (double)R : INFINITY;
    t[e] = 0;
}

__global__ __launch_bounds__(kEntryThreads) void umap_init_kernel(double* __restrict__ y, int64_t count,
                                                                  uint64_t seed) {
    const int64_t f = (int64_t)blockIdx.x * kEntryThreads + threadIdx.x;
    if (f < count) y[f] = umap_init_value(seed, (uint64_t)f);
}

template <int DIM>
__global__ __launch_bounds__(kUmapTile) void umap_epoch_kernel(int64_t n, const int64_t* __restrict__ indptr,
                                                               const int32_t* __restrict__ indices,
                                                               const double* __restrict__ eps,
                                                               double* __restrict__ eons, double* __restrict__ eonns,
                                                               uint32_t* __restrict__ t,
                                                               const double* __restrict__ y_old,
                                                               double* __restrict__ y_new, int ep, double alpha,
                                                               double a, double b, double gamma, int R,
                                                               uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * kUmapTile + threadIdx.x;
    if (i >= n) return;
    umap_vertex_epoch<DIM>(i, n, indptr, indices, eps, eons, eonns, t, y_old, y_new, ep, alpha, a, b, gamma, R, seed);
}

struct EpochArgs {
    int64_t n;
    const int64_t* indptr;
    const int32_t* indices;
    const double* eps;
    double *eons, *eonns;
    uint32_t* t;
    double *y_old, *y_new;
    int ep;
    double alpha, a, b, gamma;
    int R;
    uint64_t seed;
};

template <int DIM>
int launch_epoch(karma_ctx* ctx, const EpochArgs& g) {
    KARMA_LAUNCH(ctx, "umap_layout", umap_epoch_kernel<DIM>, (unsigned)ceil_div(g.n, kUmapTile), kUmapTile, 0, g.n,
                 g.indptr, g.indices, g.eps, g.eons, g.eonns, g.t, g.y_old, g.y_new, g.ep, g.alpha, g.a, g.b, g.gamma,
                 g.R, g.seed);
    return KARMA_OK;
}

int launch_epoch_dim(karma_ctx* ctx, int dim, const EpochArgs& g) {
    switch (dim) {
        case 1: return launch_epoch<1>(ctx, g);
        case 2: return launch_epoch<2>(ctx, g);
        case 3: return launch_epoch<3>(ctx, g);
        case 4: return launch_epoch<4>(ctx, g);
        case 5: return launch_epoch<5>(ctx, g);
        case 6: return launch_epoch<6>(ctx, g);
        case 7: return launch_epoch<7>(ctx, g);
        case 8: return launch_epoch<8>(ctx, g);
        case 9: return launch_epoch<9>(ctx, g);
        case 10: return launch_epoch<10>(ctx, g);
        case 11: return launch_epoch<11>(ctx, g);
        case 12: return launch_epoch<12>(ctx, g);
        case 13: return launch_epoch<13>(ctx, g);
        case 14: return launch_epoch<14>(ctx, g);
        case 15: return launch_epoch<15>(ctx, g);
        case 16: return launch_epoch<16>(ctx, g);
        default: KARMA_CHECK(false, KARMA_ERR_ARG, "karma_umap_layout: dim %d", dim);
    }
    return KARMA_OK;
}

// a host array's device twin, or the device array itself
template <typename T>
int on_device(karma_ctx* ctx, const T* p, size_t count, bool is_device, DevArray<T>& own, const T** out) {
    *out = p;
    if (is_device || !count) return KARMA_OK;
    KARMA_TRY(own.alloc(ctx, count));
    KARMA_HIP(hipMemcpyAsync(own.ptr, p, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *out = own.ptr;
    return KARMA_OK;
}

int key_bits_for(int64_t n) {
    int bits = 1;
    while ((int64_t(1) << bits) <= n) ++bits;
    return 32 + bits;
}

}  // namespace

extern "C" {

int karma_umap_tile(int* rows_per_block) {
    KARMA_CHECK(rows_per_block, KARMA_ERR_ARG, "karma_umap_tile: null out");
    *rows_per_block = kUmapTile;
    return KARMA_OK;
}

int karma_umap_graph(karma_ctx* ctx, const int32_t* idx, const double* dist, int64_t n, int k, int in_is_device,
                     int64_t* indptr, int32_t* indices, double* weights, int64_t cap, int64_t* nnz, double* sigma,
                     double* rho, int out_is_device) {
    UmapArgError bad = umap_graph_check_args(idx, dist, n, k, indptr, indices, weights, cap, nnz, sigma, rho);
    if (bad == kUmapArgsOk && !in_is_device) bad = umap_check_lists(idx, n, k);
    KARMA_CHECK(bad == kUmapArgsOk, KARMA_ERR_ARG, "%s", umap_arg_message(bad));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_umap_graph: null context");
    KARMA_TRY(ctx_begin(ctx));
    const int64_t E = n * k, total = 2 * E;
    const double target = std::log2((double)k);

    DevArray<int32_t> own_idx;
    DevArray<double> own_dist;
    const int32_t* idx_d = nullptr;
    const double* dist_d = nullptr;
    KARMA_TRY(on_device(ctx, idx, (size_t)E, in_is_device != 0, own_idx, &idx_d));
    KARMA_TRY(on_device(ctx, dist, (size_t)E, in_is_device != 0, own_dist, &dist_d));

    DevArray<double> rho_d, sum_d, sigma_d, memb, w_raw;
    DevArray<uint64_t> keys, skeys;
    DevArray<uint32_t> perm;
    DevArray<int> flag;
    KARMA_TRY(rho_d.alloc(ctx, n));
    KARMA_TRY(sum_d.alloc(ctx, n));
    KARMA_TRY(sigma_d.alloc(ctx, n));
    KARMA_TRY(memb.alloc(ctx, E));
    KARMA_TRY(flag.alloc(ctx, 1));
    KARMA_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), ctx->stream));

    const unsigned row_blocks = (unsigned)ceil_div(n, kUmapTile);
    KARMA_LAUNCH(ctx, "umap_graph", umap_rows_kernel, row_blocks, kUmapTile, 0, idx_d, dist_d, n, k, rho_d.ptr,
                 sum_d.ptr, flag.ptr);
    double global_mean = 0.0;
    try {
        std::vector<double> sums((size_t)n);
        int hflag = 0;
        KARMA_HIP(hipMemcpyAsync(sums.data(), sum_d.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipMemcpyAsync(&hflag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        KARMA_CHECK(hflag == 0, KARMA_ERR_ARG, "%s", umap_arg_message(kUmapArgsIndex));
        double acc = 0.0;
        for (int64_t i = 0; i < n; ++i) acc = acc + sums[(size_t)i];  // row order, from +0.0
        global_mean = acc / (double)(n * k);
    } catch (const std::bad_alloc&) {
        KARMA_CHECK(false, KARMA_ERR_OOM, "karma_umap_graph: out of host memory for %lld row sums", (long long)n);
    }

    KARMA_LAUNCH(ctx, "umap_graph", umap_sigma_kernel, row_blocks, kUmapTile, 0, idx_d, dist_d, n, k, rho_d.ptr,
                 sum_d.ptr, global_mean, target, sigma_d.ptr, memb.ptr);
    KARMA_TRY(keys.alloc(ctx, total));
    KARMA_TRY(skeys.alloc(ctx, total));
    KARMA_TRY(perm.alloc(ctx, total));
    KARMA_TRY(w_raw.alloc(ctx, total));
    KARMA_LAUNCH(ctx, "umap_graph", umap_entries_kernel, (unsigned)ceil_div(E, kEntryThreads), kEntryThreads, 0, idx_d,
                 memb.ptr, n, k, keys.ptr, w_raw.ptr);
    KARMA_TRY(radix_sort_u64(ctx, keys.ptr, nullptr, total, key_bits_for(n), skeys.ptr, perm.ptr));

    // device outputs are written in place (the caller's buffers hold 2 n k entries); host ones through twins
    DevArray<int64_t> own_ptr;
    DevArray<int32_t> own_ind;
    DevArray<double> own_w;
    int64_t* indptr_d = indptr;
    int32_t* indices_d = indices;
    double* weights_d = weights;
    if (!out_is_device) {
        KARMA_TRY(own_ptr.alloc(ctx, n + 1));
        KARMA_TRY(own_ind.alloc(ctx, total));
        KARMA_TRY(own_w.alloc(ctx, total));
        indptr_d = own_ptr.ptr, indices_d = own_ind.ptr, weights_d = own_w.ptr;
    }
    KARMA_LAUNCH(ctx, "umap_graph", umap_indptr_kernel, (unsigned)ceil_div(total + 1, kEntryThreads), kEntryThreads, 0,
                 skeys.ptr, total, n, indptr_d);
    KARMA_LAUNCH(ctx, "umap_graph", umap_gather_kernel, (unsigned)ceil_div(total, kEntryThreads), kEntryThreads, 0,
                 skeys.ptr, perm.ptr, w_raw.ptr, total, n, indices_d, weights_d);

    int64_t count = 0;
    KARMA_HIP(hipMemcpyAsync(&count, indptr_d + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    KARMA_CHECK(count >= 0 && count <= total, KARMA_ERR_STATE, "karma_umap_graph: %lld entries of at most %lld",
                (long long)count, (long long)total);
    const hipMemcpyKind kind = out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!out_is_device) {
        KARMA_HIP(hipMemcpyAsync(indptr, indptr_d, (size_t)(n + 1) * 8, kind, ctx->stream));
        if (count) {
            KARMA_HIP(hipMemcpyAsync(indices, indices_d, (size_t)count * 4, kind, ctx->stream));
            KARMA_HIP(hipMemcpyAsync(weights, weights_d, (size_t)count * 8, kind, ctx->stream));
        }
    }
    if (sigma) KARMA_HIP(hipMemcpyAsync(sigma, sigma_d.ptr, (size_t)n * 8, kind, ctx->stream));
    if (rho) KARMA_HIP(hipMemcpyAsync(rho, rho_d.ptr, (size_t)n * 8, kind, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    *nnz = count;
    return KARMA_OK;
}

int karma_umap_layout(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n,
                      int64_t nnz, int graph_is_device, int dim, double a, double b, int n_epochs,
                      int negative_sample_rate, double gamma, double initial_alpha, uint64_t seed, int init, double* y,
                      int y_is_device) {
    UmapArgError bad = umap_layout_check_args(indptr, indices, weights, n, nnz, dim, a, b, n_epochs,
                                              negative_sample_rate, gamma, initial_alpha, y);
    if (bad == kUmapArgsOk && !graph_is_device) bad = umap_check_csr(indptr, indices, weights, n, nnz);
    KARMA_CHECK(bad == kUmapArgsOk, KARMA_ERR_ARG, "%s", umap_arg_message(bad));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_umap_layout: null context");
    KARMA_TRY(ctx_begin(ctx));
    const int R = negative_sample_rate;
    const int64_t count = n * dim;

    DevArray<int64_t> own_ptr;
    DevArray<int32_t> own_ind;
    DevArray<double> own_w;
    const int64_t* indptr_d = nullptr;
    const int32_t* indices_d = nullptr;
    const double* weights_d = nullptr;
    KARMA_TRY(on_device(ctx, indptr, (size_t)(n + 1), graph_is_device != 0, own_ptr, &indptr_d));
    KARMA_TRY(on_device(ctx, indices, (size_t)nnz, graph_is_device != 0, own_ind, &indices_d));
    KARMA_TRY(on_device(ctx, weights, (size_t)nnz, graph_is_device != 0, own_w, &weights_d));

    // the graph's contents (a device graph has not been looked at yet) and the largest weight
    DevArray<int> flag;
    DevArray<unsigned long long> wmax;
    KARMA_TRY(flag.alloc(ctx, 1));
    KARMA_TRY(wmax.alloc(ctx, 1));
    KARMA_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), ctx->stream));
    KARMA_HIP(hipMemsetAsync(wmax.ptr, 0, sizeof(unsigned long long), ctx->stream));
    KARMA_LAUNCH(ctx, "umap_layout", umap_validate_kernel, (unsigned)ceil_div(std::max(n, nnz), kEntryThreads),
                 kEntryThreads, 0, indptr_d, indices_d, weights_d, n, nnz, flag.ptr, wmax.ptr);
    int hflag = 0;
    KARMA_HIP(hipMemcpyAsync(&hflag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    KARMA_CHECK(hflag == 0, KARMA_ERR_ARG, "%s",
                umap_arg_message(hflag & kBadIndptr   ? kUmapArgsIndptr
                                 : hflag & kBadColumn ? kUmapArgsColumn
                                                      : kUmapArgsWeight));

    DevArray<double> eps, eons, eonns, ya, yb;
    DevArray<uint32_t> t;
    KARMA_TRY(eps.alloc(ctx, nnz));
    KARMA_TRY(eons.alloc(ctx, nnz));
    KARMA_TRY(eonns.alloc(ctx, nnz));
    KARMA_TRY(t.alloc(ctx, nnz));
    KARMA_TRY(ya.alloc(ctx, count));
    KARMA_TRY(yb.alloc(ctx, count));
    if (nnz)
        KARMA_LAUNCH(ctx, "umap_layout", umap_schedule_kernel, (unsigned)ceil_div(nnz, kEntryThreads), kEntryThreads, 0,
                     weights_d, nnz, wmax.ptr, n_epochs, R, eps.ptr, eons.ptr, eonns.ptr, t.ptr);
    if (init) {
        KARMA_LAUNCH(ctx, "umap_layout", umap_init_kernel, (unsigned)ceil_div(count, kEntryThreads), kEntryThreads, 0,
                     ya.ptr, count, seed);
    } else {
        KARMA_HIP(hipMemcpyAsync(ya.ptr, y, (size_t)count * 8,
                                 y_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }

    EpochArgs g{n,      indptr_d, indices_d, eps.ptr, eons.ptr, eonns.ptr, t.ptr, ya.ptr,
                yb.ptr, 0,        0.0,       a,       b,        gamma,     R,     seed};
    for (int ep = 0; ep < n_epochs; ++ep) {  // no host wait in here
        g.ep = ep;
        g.alpha = initial_alpha * (1.0 - (double)ep / (double)n_epochs);
        KARMA_TRY(launch_epoch_dim(ctx, dim, g));
        std::swap(g.y_old, g.y_new);
    }
    KARMA_HIP(hipMemcpyAsync(y, g.y_old, (size_t)count * 8,
                             y_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    return KARMA_OK;
}

}  // extern "C"
