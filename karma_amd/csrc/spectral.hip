// spectral.hip — connected components of a CSR graph (karma_graph_components),
// the normalised operator S = D^-1/2 W D^-1/2 on a block (karma_spectral_apply)
// and UMAP's spectral start, component by component (karma_umap_spectral).
// Kernels "graph_components" and "umap_spectral".
//
// Components.  Labels hook to the minimum and jump to the root in rounds: a
// round's hook kernel reads the labels of the round's start and lowers the
// roots' parents with atomicMin (an integer minimum: the outcome is a set
// property), its jump kernel follows the parents, which no longer change, to
// the root.  The host reads one "changed" word per round; the rounds are
// bounded (spectral_args.h).
//
// The solver.  Vertices are laid out by (component, vertex), every component
// padded to whole tiles of kSpectralTile rows, so a tile belongs to one
// component and a tile -> component table drives all per-component work; the
// columns are relabelled once.  A block of p = dim + kSpectralGuard columns runs
// a Chebyshev-filtered subspace iteration with Rayleigh-Ritz.  The component's
// trivial vector u = sqrt(d) / |sqrt(d)| is kept as column 0 of every small
// Gram matrix, so the orthonormalisation deflates it.  Per outer round:
//   filter   kSpectralDegree operator applications, the three-term recurrence
//            in the SpMM's epilogue, the interval [-1, cut] per component
//   orth     G = [u, Y]^T [u, Y] per tile, reduced per component in tile order;
//            the host factors it, dropping dependent columns (spectral_small.h);
//            Q = [u, Y] W
//   ritz     S Q; [u, Q]^T [u, Q] and [u, Q]^T [u, S Q]; the host solves the
//            small symmetric problem by cyclic Jacobi; X = [u, Q] C,
//            S X = [u, S Q] C, residuals per tile and column; cut = the block's
//            smallest Ritz value.  A converged component is frozen: its tiles
//            are skipped by every later kernel.
// No float atomics; every sum runs in an order fixed by the shapes alone (rows
// of a tile in order, tiles of a component in order), so two calls give the
// same bytes.  The host finishes: signs, scale and the composition of y
// (include/karma.h), with umap_math.h's functions.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <new>
#include <vector>

#include "karma_internal.h"
#include "spectral_args.h"
#include "spectral_small.h"
#include "umap_math.h"

using namespace karma;

namespace {

constexpr int kThreads = 256;
constexpr int kT = kSpectralTile;
constexpr uint64_t kBlockSeedMix = 0xA0761D6478BD642Full;  // the block's start is drawn beside the layout's, not from it

enum : int { kBadIndptr = 1, kBadColumn = 2, kBadWeight = 4 };

// wall milliseconds of this thread's last karma_umap_spectral: components, reorder, solve (all of the rounds),
// and, inside the solve, the host's small dense problems (karma_spectral_last_ms)
thread_local double t_last_ms[4] = {};
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// a device graph's contents, checked before anything indexes with them (weights may be null)
__global__ __launch_bounds__(kThreads) void spec_validate_kernel(const int64_t* __restrict__ indptr,
                                                                 const int32_t* __restrict__ indices,
                                                                 const double* __restrict__ weights, int64_t n,
                                                                 int64_t nnz, int* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int flags = 0;
    if (t < n && indptr[t + 1] < indptr[t]) flags |= kBadIndptr;
    if (t == 0 && (indptr[0] != 0 || indptr[n] != nnz)) flags |= kBadIndptr;
    if (t < nnz) {
        const int32_t c = indices[t];
        if (c < 0 || (int64_t)c >= n) flags |= kBadColumn;
        if (weights) {
            const double w = weights[t];
            if (!(w > 0.0) || w == INFINITY) flags |= kBadWeight;
        }
    }
    if (flags) atomicOr(bad, flags);
}

// ---- components ---------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void cc_init_kernel(int32_t* __restrict__ lab, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) lab[i] = (int32_t)i;
}

// lab: every vertex's root at the round's start (read only); par starts as its copy
__global__ __launch_bounds__(kThreads) void cc_hook_kernel(const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int64_t n,
                                                           const int32_t* __restrict__ lab, int32_t* __restrict__ par,
                                                           int* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t li = lab[i];
    bool any = false;
    const int64_t hi = indptr[i + 1];
    for (int64_t e = indptr[i]; e < hi; ++e) {
        const int32_t lj = lab[indices[e]];
        if (lj < li) {
            atomicMin(&par[li], lj);
            any = true;
        } else if (li < lj) {
            atomicMin(&par[lj], li);
            any = true;
        }
    }
    if (any) *changed = 1;
}

// par[x] <= x and par no longer changes: the walk ends at a root after at most x steps
__global__ __launch_bounds__(kThreads) void cc_jump_kernel(const int32_t* __restrict__ par, int32_t* __restrict__ lab,
                                                           int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int32_t r = par[i];
    for (int32_t up = par[r]; up != r; up = par[r]) r = up;
    lab[i] = r;
}

// ---- the operator -------------------------------------------------------------------------

// d(i): the in-order sum from +0.0 of row i's weights; isd(i) = 1.0 / sqrt(d(i))
__global__ __launch_bounds__(kThreads) void spec_degree_kernel(const int64_t* __restrict__ indptr,
                                                               const double* __restrict__ weights, int64_t n,
                                                               double* __restrict__ d, double* __restrict__ isd) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    const int64_t hi = indptr[i + 1];
    for (int64_t e = indptr[i]; e < hi; ++e) s = s + weights[e];
    d[i] = s;
    isd[i] = 1.0 / sqrt(s);
}

// coef[e] = w * isd(j); col[e] = j, or j's row in the reordered block
__global__ __launch_bounds__(kThreads) void spec_coef_kernel(const int32_t* __restrict__ indices,
                                                             const double* __restrict__ weights,
                                                             const double* __restrict__ isd,
                                                             const int32_t* __restrict__ newpos, int64_t nnz,
                                                             int32_t* __restrict__ col, double* __restrict__ coef) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= nnz) return;
    const int32_t j = indices[e];
    coef[e] = weights[e] * isd[j];
    col[e] = newpos ? newpos[j] : j;
}

// the block's per-component tables (device copies; index: component)
struct CompTables {
    const int32_t* tile_comp;  // tile -> component
    const uint8_t* live;       // still iterating
    const int32_t* slot;       // component -> its place among the live ones of this round
    const double* centre;      // the filter's interval [-1, cut]: (cut - 1) / 2 ...
    const double* half;        // ... and (cut + 1) / 2
};

// out[r, c] = isd(i) * (sum over row i's entries in CSR order, from +0.0, of coef * x[col, c]), one thread per
// (row, column).  A row's loads do not depend on the sum: four are issued, then added in order.
// MODE 0: plain (orig == null: rows are vertices).  MODE 1: the filter's first step, (S x - centre x) / half.
// MODE 2: its later steps, 2 (S x - centre x) / half - prev.
template <int MODE>
__global__ __launch_bounds__(kThreads) void spec_spmm_kernel(int64_t rows, int p, const int64_t* __restrict__ indptr,
                                                             const int32_t* __restrict__ col,
                                                             const double* __restrict__ coef,
                                                             const double* __restrict__ isd,
                                                             const int32_t* __restrict__ orig, CompTables tab,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ prev,
                                                             double* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= rows * p) return;
    const int64_t r = f / p;
    const int c = (int)(f - r * p);
    int32_t comp = 0;
    int64_t i = r;
    if (orig) {
        comp = tab.tile_comp[r / kT];
        if (!tab.live[comp]) return;
        i = orig[r];
        if (i < 0) return;  // a padding row: zero since the buffers were cleared
    }
    const int64_t hi = indptr[i + 1];
    int64_t e = indptr[i];
    double sum = 0.0;
    for (; e + 4 <= hi; e += 4) {
        const double t0 = coef[e] * x[(int64_t)col[e] * p + c];
        const double t1 = coef[e + 1] * x[(int64_t)col[e + 1] * p + c];
        const double t2 = coef[e + 2] * x[(int64_t)col[e + 2] * p + c];
        const double t3 = coef[e + 3] * x[(int64_t)col[e + 3] * p + c];
        sum = sum + t0;
        sum = sum + t1;
        sum = sum + t2;
        sum = sum + t3;
    }
    for (; e < hi; ++e) sum = sum + coef[e] * x[(int64_t)col[e] * p + c];
    double v = hi > indptr[i] ? isd[i] * sum : 0.0;  // an empty row: +0.0, not inf * 0
    if (MODE != 0) {
        v = (v - tab.centre[comp] * x[f]) / tab.half[comp];
        if (MODE == 2) v = 2.0 * v - prev[f];
    }
    out[f] = v;
}

// ---- the block ----------------------------------------------------------------------------

// x[r, c]: the counter generator's value of (vertex, column) scaled to [-1, 1); u[r] = sqrt(d) / unorm; padding: 0
__global__ __launch_bounds__(kThreads) void spec_start_kernel(int64_t rows, int p, const int32_t* __restrict__ orig,
                                                              CompTables tab, const double* __restrict__ d,
                                                              const double* __restrict__ unorm, uint64_t seed,
                                                              double* __restrict__ x, double* __restrict__ u) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= rows * p) return;
    const int64_t r = f / p;
    const int c = (int)(f - r * p);
    const int32_t comp = tab.tile_comp[r / kT];
    const int64_t i = orig[r];
    const bool real = i >= 0 && tab.live[comp];
    x[f] = real ? umap_init_value(seed, (uint64_t)(i * p + c)) / 10.0 : 0.0;
    if (c == 0) u[r] = real ? sqrt(d[i]) / unorm[comp] : 0.0;
}

// part[tile][i * P + j] = sum over the tile's rows in order of [u, a][r, i] * [u, b][r, j]
__global__ __launch_bounds__(kThreads) void spec_gram_kernel(int p, CompTables tab, const double* __restrict__ u,
                                                             const double* __restrict__ a,
                                                             const double* __restrict__ b,
                                                             double* __restrict__ part) {
    __shared__ double sa[kT * kSpectralBasisMax];
    __shared__ double sb[kT * kSpectralBasisMax];
    const int64_t tile = blockIdx.x;
    if (!tab.live[tab.tile_comp[tile]]) return;  // uniform over the block
    const int P = p + 1;
    for (int t = threadIdx.x; t < kT * P; t += kThreads) {
        const int r = t / P, k = t - r * P;
        const int64_t row = tile * kT + r;
        sa[t] = k == 0 ? u[row] : a[row * p + (k - 1)];
        sb[t] = k == 0 ? u[row] : b[row * p + (k - 1)];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < P * P; t += kThreads) {
        const int i = t / P, j = t - i * P;
        double s = 0.0;
        for (int r = 0; r < kT; ++r) s = s + sa[r * P + i] * sb[r * P + j];
        part[tile * (int64_t)(P * P) + t] = s;
    }
}

// out[slot][e] = the sum over the component's tiles in order of part[tile][e]; one block row per live component
__global__ __launch_bounds__(kThreads) void spec_reduce_kernel(int width, const int32_t* __restrict__ act,
                                                               const int64_t* __restrict__ tile0,
                                                               const double* __restrict__ part,
                                                               double* __restrict__ out) {
    const int e = blockIdx.y * kThreads + threadIdx.x;
    if (e >= width) return;
    const int32_t comp = act[blockIdx.x];
    const int64_t lo = tile0[comp], hi = tile0[comp + 1];
    double s = 0.0;
    int64_t t = lo;
    for (; t + 4 <= hi; t += 4) {
        const double v0 = part[t * width + e], v1 = part[(t + 1) * width + e];
        const double v2 = part[(t + 2) * width + e], v3 = part[(t + 3) * width + e];
        s = s + v0;
        s = s + v1;
        s = s + v2;
        s = s + v3;
    }
    for (; t < hi; ++t) s = s + part[t * width + e];
    out[(int64_t)blockIdx.x * width + e] = s;
}

// out[r, c] = u[r] * w[0, c] + sum over k in order of a[r, k] * w[k + 1, c]; w: the component's P x p matrix
__global__ __launch_bounds__(kThreads) void spec_combine_kernel(int64_t rows, int p, CompTables tab,
                                                                const double* __restrict__ u,
                                                                const double* __restrict__ a,
                                                                const double* __restrict__ w,
                                                                double* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= rows * p) return;
    const int64_t r = f / p;
    const int c = (int)(f - r * p);
    const int32_t comp = tab.tile_comp[r / kT];
    if (!tab.live[comp]) return;
    const double* m = w + (int64_t)tab.slot[comp] * (p + 1) * p;
    double s = u[r] * m[c];
    for (int k = 0; k < p; ++k) s = s + a[r * p + k] * m[(k + 1) * p + c];
    out[f] = s;
}

// part[tile][c] = sum over the tile's rows in order of (sx[r, c] - theta[c] * x[r, c])^2
__global__ __launch_bounds__(kT) void spec_resid_kernel(int p, CompTables tab, const double* __restrict__ x,
                                                        const double* __restrict__ sx,
                                                        const double* __restrict__ theta,
                                                        double* __restrict__ part) {
    const int64_t tile = blockIdx.x;
    const int32_t comp = tab.tile_comp[tile];
    const int c = threadIdx.x;
    if (!tab.live[comp] || c >= p) return;
    const double th = theta[(int64_t)tab.slot[comp] * p + c];
    double s = 0.0;
    for (int r = 0; r < kT; ++r) {
        const int64_t at = (tile * kT + r) * p + c;
        const double e = sx[at] - th * x[at];
        s = s + e * e;
    }
    part[tile * p + c] = s;
}

// ---- host side ----------------------------------------------------------------------------

template <typename T>
int on_device(karma_ctx* ctx, const T* p, size_t count, bool is_device, DevArray<T>& own, const T** out) {
    *out = p;
    if (is_device || !count) return KARMA_OK;
    KARMA_TRY(own.alloc(ctx, count));
    KARMA_HIP(hipMemcpyAsync(own.ptr, p, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *out = own.ptr;
    return KARMA_OK;
}

template <typename T>
int upload(karma_ctx* ctx, DevArray<T>& dst, const std::vector<T>& src) {
    if (dst.n < src.size() || !dst.ptr) KARMA_TRY(dst.alloc(ctx, src.size()));
    if (!src.empty())
        KARMA_HIP(hipMemcpyAsync(dst.ptr, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return KARMA_OK;
}

struct Graph {
    int64_t n = 0, nnz = 0;
    DevArray<int64_t> own_ptr;
    DevArray<int32_t> own_ind;
    DevArray<double> own_w;
    const int64_t* indptr = nullptr;
    const int32_t* indices = nullptr;
    const double* weights = nullptr;
};

// the graph on the device, its contents checked there where it came from there
int graph_open(karma_ctx* ctx, const char* who, const int64_t* indptr, const int32_t* indices, const double* weights,
               int64_t n, int64_t nnz, bool is_device, Graph& g) {
    g.n = n, g.nnz = nnz;
    KARMA_TRY(on_device(ctx, indptr, (size_t)(n + 1), is_device, g.own_ptr, &g.indptr));
    KARMA_TRY(on_device(ctx, indices, (size_t)nnz, is_device, g.own_ind, &g.indices));
    if (weights) KARMA_TRY(on_device(ctx, weights, (size_t)nnz, is_device, g.own_w, &g.weights));
    if (!is_device) return KARMA_OK;  // a host graph was checked before the device was looked for
    DevArray<int> flag;
    KARMA_TRY(flag.alloc(ctx, 1));
    KARMA_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), ctx->stream));
    KARMA_LAUNCH(ctx, who, spec_validate_kernel, (unsigned)ceil_div(std::max(n + 1, nnz), kThreads), kThreads, 0,
                 g.indptr, g.indices, g.weights, n, nnz, flag.ptr);
    int hflag = 0;
    KARMA_HIP(hipMemcpyAsync(&hflag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    KARMA_CHECK(hflag == 0, KARMA_ERR_ARG, "%s",
                umap_arg_message(hflag & kBadIndptr   ? kUmapArgsIndptr
                                 : hflag & kBadColumn ? kUmapArgsColumn
                                                      : kUmapArgsWeight));
    return KARMA_OK;
}

// lab (device, int32[n]): every vertex's smallest component member
int components_run(karma_ctx* ctx, const Graph& g, int32_t* lab) {
    const int64_t n = g.n;
    const unsigned blocks = (unsigned)ceil_div(n, kThreads);
    DevArray<int32_t> par;
    DevArray<int> changed;
    KARMA_TRY(par.alloc(ctx, n));
    KARMA_TRY(changed.alloc(ctx, 1));
    KARMA_LAUNCH(ctx, "graph_components", cc_init_kernel, blocks, kThreads, 0, lab, n);
    const int bound = components_rounds_max(n);
    for (int round = 0;; ++round) {
        KARMA_CHECK(round < bound, KARMA_ERR_STATE, "karma_graph_components: not settled after %d rounds", bound);
        KARMA_HIP(hipMemsetAsync(changed.ptr, 0, sizeof(int), ctx->stream));
        KARMA_HIP(hipMemcpyAsync(par.ptr, lab, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        KARMA_LAUNCH(ctx, "graph_components", cc_hook_kernel, blocks, kThreads, 0, g.indptr, g.indices, n, lab, par.ptr,
                     changed.ptr);
        int h = 0;
        KARMA_HIP(hipMemcpyAsync(&h, changed.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        if (!h) break;
        KARMA_LAUNCH(ctx, "graph_components", cc_jump_kernel, blocks, kThreads, 0, par.ptr, lab, n);
    }
    return KARMA_OK;
}

int components_impl(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz,
                    bool graph_is_device, int32_t* comp, bool comp_is_device, int64_t* n_comp) {
    Graph g;
    KARMA_TRY(graph_open(ctx, "graph_components", indptr, indices, nullptr, n, nnz, graph_is_device, g));
    DevArray<int32_t> own;
    int32_t* lab = comp;
    if (!comp_is_device) {
        KARMA_TRY(own.alloc(ctx, n));
        lab = own.ptr;
    }
    KARMA_TRY(components_run(ctx, g, lab));
    std::vector<int32_t> host;
    int32_t* h = comp;
    if (comp_is_device) {
        host.resize((size_t)n);
        h = host.data();
    }
    KARMA_HIP(hipMemcpyAsync(h, lab, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    int64_t count = 0;
    for (int64_t i = 0; i < n; ++i) count += h[i] == (int32_t)i;
    *n_comp = count;
    return KARMA_OK;
}

// d and isd of every row
int degrees_run(karma_ctx* ctx, const Graph& g, DevArray<double>& d, DevArray<double>& isd) {
    KARMA_TRY(d.alloc(ctx, g.n));
    KARMA_TRY(isd.alloc(ctx, g.n));
    KARMA_LAUNCH(ctx, "umap_spectral", spec_degree_kernel, (unsigned)ceil_div(g.n, kThreads), kThreads, 0, g.indptr,
                 g.weights, g.n, d.ptr, isd.ptr);
    return KARMA_OK;
}

// the entries' coefficients and columns (newpos != null: relabelled to the reordered block's rows)
int coefficients_run(karma_ctx* ctx, const Graph& g, const double* isd, const int32_t* newpos, DevArray<int32_t>& col,
                     DevArray<double>& coef) {
    KARMA_TRY(col.alloc(ctx, g.nnz));
    KARMA_TRY(coef.alloc(ctx, g.nnz));
    if (g.nnz)
        KARMA_LAUNCH(ctx, "umap_spectral", spec_coef_kernel, (unsigned)ceil_div(g.nnz, kThreads), kThreads, 0,
                     g.indices, g.weights, isd, newpos, g.nnz, col.ptr, coef.ptr);
    return KARMA_OK;
}

int apply_impl(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n,
               int64_t nnz, bool graph_is_device, const double* x, int p, double* out, bool x_is_device) {
    Graph g;
    KARMA_TRY(graph_open(ctx, "umap_spectral", indptr, indices, weights, n, nnz, graph_is_device, g));
    DevArray<double> d, isd, coef, own_x, own_out;
    DevArray<int32_t> col;
    KARMA_TRY(degrees_run(ctx, g, d, isd));
    KARMA_TRY(coefficients_run(ctx, g, isd.ptr, nullptr, col, coef));
    const double* x_d = nullptr;
    KARMA_TRY(on_device(ctx, x, (size_t)(n * p), x_is_device, own_x, &x_d));
    double* out_d = out;
    if (!x_is_device) {
        KARMA_TRY(own_out.alloc(ctx, n * p));
        out_d = own_out.ptr;
    }
    KARMA_LAUNCH(ctx, "umap_spectral", spec_spmm_kernel<0>, (unsigned)ceil_div(n * p, kThreads), kThreads, 0, n, p,
                 g.indptr, col.ptr, coef.ptr, isd.ptr, (const int32_t*)nullptr, CompTables{}, x_d,
                 (const double*)nullptr, out_d);
    if (!x_is_device)
        KARMA_HIP(hipMemcpyAsync(out, out_d, (size_t)(n * p) * 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    return KARMA_OK;
}

// one component of the solve (host)
struct Comp {
    int32_t root = 0;   // smallest vertex
    int64_t size = 0;   // s
    int m = 0;          // min(dim, s - 1)
    bool live = false;  // still iterating
    bool converged = false;
    double cut = 0.0;
};

int spectral_impl(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n,
                  int64_t nnz, bool graph_is_device, int dim, uint64_t seed, double tol, int max_outer, double* y,
                  double* vec, double* lam, double* res, int32_t* comp, bool out_is_device, int64_t* info) {
    Graph g;
    KARMA_TRY(graph_open(ctx, "umap_spectral", indptr, indices, weights, n, nnz, graph_is_device, g));
    const int p = dim + kSpectralGuard, P = p + 1, PP = P * P;

    // ---- components and the layout of the block
    for (double& t : t_last_ms) t = 0.0;
    double mark = now_ms();
    DevArray<int32_t> lab_d;
    KARMA_TRY(lab_d.alloc(ctx, n));
    KARMA_TRY(components_run(ctx, g, lab_d.ptr));
    t_last_ms[0] = now_ms() - mark;
    mark = now_ms();
    DevArray<double> d_d, isd_d, coef_d;
    DevArray<int32_t> col_d;
    KARMA_TRY(degrees_run(ctx, g, d_d, isd_d));
    std::vector<int32_t> lab((size_t)n);
    std::vector<double> deg((size_t)n);
    KARMA_HIP(hipMemcpyAsync(lab.data(), lab_d.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipMemcpyAsync(deg.data(), d_d.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));

    std::vector<int32_t> cid((size_t)n, -1);  // root vertex -> component number (by ascending root)
    std::vector<Comp> comps;
    for (int64_t i = 0; i < n; ++i)
        if (lab[(size_t)i] == (int32_t)i) {
            cid[(size_t)i] = (int32_t)comps.size();
            comps.emplace_back();
            comps.back().root = (int32_t)i;
        }
    const int64_t nc = (int64_t)comps.size();
    for (int64_t i = 0; i < n; ++i) comps[(size_t)cid[(size_t)lab[(size_t)i]]].size += 1;
    std::vector<int64_t> tile0((size_t)nc + 1, 0);
    std::vector<double> unorm((size_t)nc, 0.0);
    for (int64_t c = 0; c < nc; ++c) {
        Comp& k = comps[(size_t)c];
        k.m = (int)std::min<int64_t>(dim, k.size - 1);
        k.live = k.size >= 2;
        k.converged = !k.live;  // a single vertex has nothing to find
        tile0[(size_t)c + 1] = tile0[(size_t)c] + ceil_div(k.size, kT);
    }
    const int64_t tiles = tile0[(size_t)nc], rows = tiles * kT;
    KARMA_CHECK(rows * p <= kSpectralMaxCells, KARMA_ERR_ARG, "%s", spectral_arg_message(kSpectralArgsBytes));
    std::vector<int32_t> newpos((size_t)n), orig((size_t)rows, -1), tile_comp((size_t)tiles);
    {
        std::vector<int64_t> cursor((size_t)nc);
        for (int64_t c = 0; c < nc; ++c) {
            cursor[(size_t)c] = tile0[(size_t)c] * kT;
            for (int64_t t = tile0[(size_t)c]; t < tile0[(size_t)c + 1]; ++t) tile_comp[(size_t)t] = (int32_t)c;
        }
        for (int64_t i = 0; i < n; ++i) {  // ascending vertex within a component
            const int32_t c = cid[(size_t)lab[(size_t)i]];
            const int64_t r = cursor[(size_t)c]++;
            newpos[(size_t)i] = (int32_t)r;
            orig[(size_t)r] = (int32_t)i;
            unorm[(size_t)c] = unorm[(size_t)c] + deg[(size_t)i];
        }
        for (int64_t c = 0; c < nc; ++c) unorm[(size_t)c] = std::sqrt(unorm[(size_t)c]);
    }
    KARMA_CHECK(rows < kKnnMaxRows, KARMA_ERR_ARG, "%s", spectral_arg_message(kSpectralArgsBytes));

    DevArray<int32_t> newpos_d, orig_d, tile_comp_d, slot_d, act_d;
    DevArray<int64_t> tile0_d;
    DevArray<uint8_t> live_d;
    DevArray<double> unorm_d, centre_d, half_d;
    KARMA_TRY(upload(ctx, newpos_d, newpos));
    KARMA_TRY(upload(ctx, orig_d, orig));
    KARMA_TRY(upload(ctx, tile_comp_d, tile_comp));
    KARMA_TRY(upload(ctx, tile0_d, tile0));
    KARMA_TRY(upload(ctx, unorm_d, unorm));
    KARMA_TRY(coefficients_run(ctx, g, isd_d.ptr, newpos_d.ptr, col_d, coef_d));

    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    t_last_ms[1] = now_ms() - mark;
    mark = now_ms();

    // ---- the block
    const int64_t cells = rows * p;
    const unsigned cell_blocks = (unsigned)ceil_div(cells, kThreads);
    DevArray<double> x_d, u_d, tmp_d[3], part_d, red_d, small_d, theta_d;
    KARMA_TRY(x_d.alloc(ctx, cells));
    KARMA_TRY(u_d.alloc(ctx, rows));
    for (auto& t : tmp_d) {
        KARMA_TRY(t.alloc(ctx, cells));
        KARMA_HIP(hipMemsetAsync(t.ptr, 0, (size_t)cells * 8, ctx->stream));  // padding rows stay +0.0
    }
    KARMA_TRY(part_d.alloc(ctx, tiles * PP));

    std::vector<uint8_t> live((size_t)nc);
    std::vector<int32_t> slot((size_t)nc, 0), act;
    std::vector<double> centre((size_t)nc, 0.0), half((size_t)nc, 1.0);
    auto tables = [&]() {
        return CompTables{tile_comp_d.ptr, live_d.ptr, slot_d.ptr, centre_d.ptr, half_d.ptr};
    };
    auto refresh = [&]() -> int {  // the live components of the coming round
        act.clear();
        for (int64_t c = 0; c < nc; ++c) {
            live[(size_t)c] = comps[(size_t)c].live;
            slot[(size_t)c] = (int32_t)act.size();
            if (comps[(size_t)c].live) act.push_back((int32_t)c);
        }
        KARMA_TRY(upload(ctx, live_d, live));
        KARMA_TRY(upload(ctx, slot_d, slot));
        KARMA_TRY(upload(ctx, act_d, act));
        KARMA_TRY(upload(ctx, centre_d, centre));
        KARMA_TRY(upload(ctx, half_d, half));
        return KARMA_OK;
    };
    KARMA_TRY(refresh());
    KARMA_LAUNCH(ctx, "umap_spectral", spec_start_kernel, cell_blocks, kThreads, 0, rows, p, orig_d.ptr, tables(),
                 d_d.ptr, unorm_d.ptr, seed ^ kBlockSeedMix, x_d.ptr, u_d.ptr);

    // per-component results (index: component, column)
    std::vector<double> c_lam((size_t)nc * dim, 0.0), c_res((size_t)nc * dim, 0.0);
    std::vector<double> gram, gram2, hmat, wmat, theta, resid;
    int64_t rounds = 0, applications = 0;

    // the sum of the tiles' partials per live component, on the host
    auto reduce_to_host = [&](int width, std::vector<double>& out) -> int {
        const int64_t na = (int64_t)act.size();
        if (red_d.n < (size_t)(na * width) || !red_d.ptr) KARMA_TRY(red_d.alloc(ctx, na * width));
        KARMA_LAUNCH(ctx, "umap_spectral", spec_reduce_kernel, dim3((unsigned)na, (unsigned)ceil_div(width, kThreads)),
                     kThreads, 0, width, act_d.ptr, tile0_d.ptr, part_d.ptr, red_d.ptr);
        out.resize((size_t)(na * width));
        KARMA_HIP(hipMemcpyAsync(out.data(), red_d.ptr, (size_t)(na * width) * 8, hipMemcpyDeviceToHost, ctx->stream));
        KARMA_HIP(hipStreamSynchronize(ctx->stream));
        return KARMA_OK;
    };
    auto spmm = [&](int mode, const double* in, const double* prev, double* out) -> int {
        ++applications;
        if (mode == 0)
            KARMA_LAUNCH(ctx, "umap_spectral", spec_spmm_kernel<0>, cell_blocks, kThreads, 0, rows, p, g.indptr,
                         col_d.ptr, coef_d.ptr, isd_d.ptr, orig_d.ptr, tables(), in, prev, out);
        else if (mode == 1)
            KARMA_LAUNCH(ctx, "umap_spectral", spec_spmm_kernel<1>, cell_blocks, kThreads, 0, rows, p, g.indptr,
                         col_d.ptr, coef_d.ptr, isd_d.ptr, orig_d.ptr, tables(), in, prev, out);
        else
            KARMA_LAUNCH(ctx, "umap_spectral", spec_spmm_kernel<2>, cell_blocks, kThreads, 0, rows, p, g.indptr,
                         col_d.ptr, coef_d.ptr, isd_d.ptr, orig_d.ptr, tables(), in, prev, out);
        return KARMA_OK;
    };

    for (int round = 0; round < max_outer && !act.empty(); ++round) {
        ++rounds;
        const int64_t na = (int64_t)act.size();
        // filter: the block's first round has no Ritz values yet and goes straight to Rayleigh-Ritz
        // (step k of the recurrence writes buffer (k - 1) mod 3 from buffers (k - 2) and (k - 3) mod 3)
        double* f = x_d.ptr;
        double *t0 = tmp_d[0].ptr, *t1 = tmp_d[1].ptr, *t2 = tmp_d[2].ptr;
        if (round > 0) {
            static_assert(kSpectralDegree >= 2, "the recurrence's first two steps are written out");
            KARMA_TRY(spmm(1, x_d.ptr, nullptr, tmp_d[0].ptr));
            KARMA_TRY(spmm(2, tmp_d[0].ptr, x_d.ptr, tmp_d[1].ptr));
            for (int k = 3; k <= kSpectralDegree; ++k)
                KARMA_TRY(spmm(2, tmp_d[(k - 2) % 3].ptr, tmp_d[(k - 3) % 3].ptr, tmp_d[(k - 1) % 3].ptr));
            constexpr int last = (kSpectralDegree - 1) % 3;
            f = tmp_d[last].ptr;
            t0 = tmp_d[(last + 1) % 3].ptr;
            t1 = tmp_d[(last + 2) % 3].ptr;
            t2 = f;  // free once Q is built
        }
        // orth: Q = [u, f] W into t0
        KARMA_LAUNCH(ctx, "umap_spectral", spec_gram_kernel, (unsigned)tiles, kThreads, 0, p, tables(), u_d.ptr, f, f,
                     part_d.ptr);
        KARMA_TRY(reduce_to_host(PP, gram));
        wmat.assign((size_t)(na * P * p), 0.0);
        double small_mark = now_ms();
#pragma omp parallel for schedule(dynamic, 16)
        for (int64_t a = 0; a < na; ++a) spectral_orth(&gram[(size_t)(a * PP)], P, &wmat[(size_t)(a * P * p)]);
        t_last_ms[3] += now_ms() - small_mark;
        KARMA_TRY(upload(ctx, small_d, wmat));
        KARMA_LAUNCH(ctx, "umap_spectral", spec_combine_kernel, cell_blocks, kThreads, 0, rows, p, tables(), u_d.ptr, f,
                     small_d.ptr, t0);
        // ritz: S Q into t1
        KARMA_TRY(spmm(0, t0, nullptr, t1));
        KARMA_LAUNCH(ctx, "umap_spectral", spec_gram_kernel, (unsigned)tiles, kThreads, 0, p, tables(), u_d.ptr, t0, t0,
                     part_d.ptr);
        KARMA_TRY(reduce_to_host(PP, gram2));
        KARMA_LAUNCH(ctx, "umap_spectral", spec_gram_kernel, (unsigned)tiles, kThreads, 0, p, tables(), u_d.ptr, t0, t1,
                     part_d.ptr);
        KARMA_TRY(reduce_to_host(PP, hmat));
        theta.assign((size_t)(na * p), kSpectralNoRitz);
        std::vector<int> kept((size_t)na, 0);
        small_mark = now_ms();
#pragma omp parallel for schedule(dynamic, 16)
        for (int64_t a = 0; a < na; ++a)
            kept[(size_t)a] = spectral_ritz(&gram2[(size_t)(a * PP)], &hmat[(size_t)(a * PP)], P,
                                            &wmat[(size_t)(a * P * p)], &theta[(size_t)(a * p)]);
        t_last_ms[3] += now_ms() - small_mark;
        KARMA_TRY(upload(ctx, small_d, wmat));
        KARMA_TRY(upload(ctx, theta_d, theta));
        // S X = [u, S Q] C into the third buffer (the filter's result, no longer needed); X = [u, Q] C in place of the
        // old block
        double* sx = t2;
        KARMA_LAUNCH(ctx, "umap_spectral", spec_combine_kernel, cell_blocks, kThreads, 0, rows, p, tables(), u_d.ptr, t1,
                     small_d.ptr, sx);
        KARMA_LAUNCH(ctx, "umap_spectral", spec_combine_kernel, cell_blocks, kThreads, 0, rows, p, tables(), u_d.ptr, t0,
                     small_d.ptr, x_d.ptr);
        KARMA_LAUNCH(ctx, "umap_spectral", spec_resid_kernel, (unsigned)tiles, kT, 0, p, tables(), x_d.ptr, sx,
                     theta_d.ptr, part_d.ptr);
        KARMA_TRY(reduce_to_host(p, resid));
        for (int64_t a = 0; a < na; ++a) {
            Comp& k = comps[(size_t)act[(size_t)a]];
            const int q = kept[(size_t)a];
            bool ok = q >= k.m;
            for (int c = 0; c < k.m; ++c) {
                const double r = c < q ? std::sqrt(resid[(size_t)(a * p + c)]) : INFINITY;
                c_lam[(size_t)act[(size_t)a] * dim + c] = c < q ? 1.0 - theta[(size_t)(a * p + c)] : 0.0;
                c_res[(size_t)act[(size_t)a] * dim + c] = r;
                ok = ok && r <= tol;
            }
            if (ok) {
                k.converged = true;
                k.live = false;
            } else if (q > 0) {  // damp [-1, the block's smallest Ritz value]
                double cut = theta[(size_t)(a * p + q - 1)];
                cut = cut < -0.9 ? -0.9 : (cut > 0.9999999 ? 0.9999999 : cut);
                centre[(size_t)act[(size_t)a]] = (cut - 1.0) / 2.0;
                half[(size_t)act[(size_t)a]] = (cut + 1.0) / 2.0;
            }
        }
        KARMA_TRY(refresh());
    }

    t_last_ms[2] = now_ms() - mark;

    // ---- the host's finish: signs, scale, composition
    std::vector<double> xh((size_t)cells);
    KARMA_HIP(hipMemcpyAsync(xh.data(), x_d.ptr, (size_t)cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    const size_t count = (size_t)n * dim;
    std::vector<double> yv(count), vv(count, 0.0), lv, rv;
    if (lam) lv.assign(count, 0.0);
    if (res) rv.assign(count, 0.0);
    int64_t failed = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : failed)
    for (int64_t c = 0; c < nc; ++c) {
        const Comp& k = comps[(size_t)c];
        const int64_t r0 = tile0[(size_t)c] * kT;
        double vmax = 0.0;
        for (int col = 0; col < k.m; ++col) {
            double big = 0.0, sign = 1.0;
            for (int64_t r = r0; r < r0 + k.size; ++r) {  // the entry of largest magnitude, first by vertex
                const double v = xh[(size_t)(r * p + col)];
                if (std::fabs(v) > big) big = std::fabs(v), sign = v < 0.0 ? -1.0 : 1.0;
            }
            for (int64_t r = r0; r < r0 + k.size; ++r) {
                const double v = xh[(size_t)(r * p + col)];
                vv[(size_t)orig[(size_t)r] * dim + col] = sign < 0.0 ? -v : v;
            }
            vmax = big > vmax ? big : vmax;
            if (lam) lv[(size_t)k.root * dim + col] = c_lam[(size_t)c * dim + col];
            if (res) rv[(size_t)k.root * dim + col] = c_res[(size_t)c * dim + col];
        }
        if (!k.converged) failed += 1;
        const double share = (double)k.size / (double)n;
        const double radius = 10.0 * kpow(share, 1.0 / (double)dim);
        const double scale = k.m > 0 ? radius / vmax : 0.0;
        for (int64_t r = r0; r < r0 + k.size; ++r) {
            const uint64_t i = (uint64_t)orig[(size_t)r];
            for (int col = 0; col < dim; ++col) {
                const uint64_t flat = i * (uint64_t)dim + (uint64_t)col;
                double v;
                if (!k.converged) {
                    v = umap_init_value(seed, flat);
                } else {
                    v = umap_init_value(seed, (uint64_t)k.root * (uint64_t)dim + (uint64_t)col) * (1.0 - share);
                    if (col < k.m) v = v + scale * vv[flat];
                    v = v + 1e-4 * (-1.0 + 2.0 * (((double)(splitmix64(seed + 1 + (flat + 1) * kUmapGolden) >> 11)) *
                                                  0x1p-53));
                }
                yv[flat] = v;
            }
        }
    }

    const hipMemcpyKind kind = out_is_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
    KARMA_HIP(hipMemcpyAsync(y, yv.data(), count * 8, kind, ctx->stream));
    if (vec) KARMA_HIP(hipMemcpyAsync(vec, vv.data(), count * 8, kind, ctx->stream));
    if (lam) KARMA_HIP(hipMemcpyAsync(lam, lv.data(), count * 8, kind, ctx->stream));
    if (res) KARMA_HIP(hipMemcpyAsync(res, rv.data(), count * 8, kind, ctx->stream));
    if (comp) KARMA_HIP(hipMemcpyAsync(comp, lab.data(), (size_t)n * 4, kind, ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    info[0] = nc;
    info[1] = failed;
    info[2] = rounds;
    info[3] = applications;
    return KARMA_OK;
}

const char* csr_or_args(SpectralArgError e, UmapArgError u) {
    return e != kSpectralArgsOk ? spectral_arg_message(e) : umap_arg_message(u);
}

}  // namespace

extern "C" {

int karma_spectral_tile(int* rows_per_tile, int* guard, int* degree) {
    KARMA_CHECK(rows_per_tile && guard && degree, KARMA_ERR_ARG, "karma_spectral_tile: null out");
    *rows_per_tile = kSpectralTile;
    *guard = kSpectralGuard;
    *degree = kSpectralDegree;
    return KARMA_OK;
}

int karma_spectral_last_ms(double* ms) {
    KARMA_CHECK(ms, KARMA_ERR_ARG, "karma_spectral_last_ms: null out");
    for (int i = 0; i < 4; ++i) ms[i] = t_last_ms[i];
    return KARMA_OK;
}

int karma_spectral_jacobi(const double* a, int p, double* w, double* v) {
    KARMA_CHECK(a && w && v, KARMA_ERR_ARG, "karma_spectral_jacobi: null pointer");
    KARMA_CHECK(p >= 1 && p <= kSpectralBasisMax, KARMA_ERR_ARG, "karma_spectral_jacobi: need 1 <= p <= %d",
                kSpectralBasisMax);
    double work[kSpectralBasisMax * kSpectralBasisMax];
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) work[i * p + j] = 0.5 * (a[i * p + j] + a[j * p + i]);
    KARMA_CHECK(spectral_jacobi(work, p, w, v) < kSpectralSweepsMax, KARMA_ERR_STATE,
                "karma_spectral_jacobi: not settled after %d sweeps", kSpectralSweepsMax);
    return KARMA_OK;
}

int karma_graph_components(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz,
                           int graph_is_device, int32_t* comp, int comp_is_device, int64_t* n_comp) {
    const SpectralArgError bad = components_check_args(indptr, indices, n, nnz, comp, n_comp);
    UmapArgError csr = kUmapArgsOk;
    if (bad == kSpectralArgsOk && !graph_is_device) csr = spectral_check_csr(indptr, indices, nullptr, n, nnz);
    KARMA_CHECK(bad == kSpectralArgsOk && csr == kUmapArgsOk, KARMA_ERR_ARG, "%s", csr_or_args(bad, csr));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_graph_components: null context");
    KARMA_TRY(ctx_begin(ctx));
    try {
        return components_impl(ctx, indptr, indices, n, nnz, graph_is_device != 0, comp, comp_is_device != 0, n_comp);
    } catch (const std::bad_alloc&) {
        KARMA_CHECK(false, KARMA_ERR_OOM, "karma_graph_components: out of host memory");
    }
}

int karma_spectral_apply(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights,
                         int64_t n, int64_t nnz, int graph_is_device, const double* x, int p, double* out,
                         int x_is_device) {
    const SpectralArgError bad = apply_check_args(indptr, indices, weights, n, nnz, x, p, out);
    UmapArgError csr = kUmapArgsOk;
    if (bad == kSpectralArgsOk && !graph_is_device) csr = spectral_check_csr(indptr, indices, weights, n, nnz);
    KARMA_CHECK(bad == kSpectralArgsOk && csr == kUmapArgsOk, KARMA_ERR_ARG, "%s", csr_or_args(bad, csr));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_spectral_apply: null context");
    KARMA_TRY(ctx_begin(ctx));
    return apply_impl(ctx, indptr, indices, weights, n, nnz, graph_is_device != 0, x, p, out, x_is_device != 0);
}

int karma_umap_spectral(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights,
                        int64_t n, int64_t nnz, int graph_is_device, int dim, uint64_t seed, double tol, int max_outer,
                        double* y, double* vec, double* lam, double* res, int32_t* comp, int out_is_device,
                        int64_t* info) {
    const SpectralArgError bad =
        spectral_check_args(indptr, indices, weights, n, nnz, dim, tol, max_outer, y, vec, lam, res, comp, info);
    UmapArgError csr = kUmapArgsOk;
    if (bad == kSpectralArgsOk && !graph_is_device) csr = spectral_check_csr(indptr, indices, weights, n, nnz);
    KARMA_CHECK(bad == kSpectralArgsOk && csr == kUmapArgsOk, KARMA_ERR_ARG, "%s", csr_or_args(bad, csr));
    KARMA_CHECK(ctx, KARMA_ERR_ARG, "karma_umap_spectral: null context");
    KARMA_TRY(ctx_begin(ctx));
    try {
        return spectral_impl(ctx, indptr, indices, weights, n, nnz, graph_is_device != 0, dim, seed, tol, max_outer, y,
                             vec, lam, res, comp, out_is_device != 0, info);
    } catch (const std::bad_alloc&) {
        KARMA_CHECK(false, KARMA_ERR_OOM, "karma_umap_spectral: out of host memory");
    }
}

}  // extern "C"
