// spectral_args.h — the argument checks, tile constants and round bound of
// karma_graph_components, karma_spectral_apply and karma_umap_spectral: a pure
// host header (no HIP), shared by spectral.hip and spectral_args_test.cpp.  The
// CSR contents of a host graph are checked by umap_check_csr (umap_args.h).
#pragma once

#include <cmath>
#include <cstdint>

#include "umap_args.h"

namespace karma {

constexpr int kSpectralTile = 64;    // rows per tile of the reordered block; a tile belongs to one component
constexpr int kSpectralGuard = 6;    // columns of the block beyond dim
constexpr int kSpectralDegree = 12;  // degree of the Chebyshev filter
constexpr int kSpectralColsMax = 32; // columns karma_spectral_apply takes
constexpr int64_t kSpectralMaxCells = int64_t(1) << 38;  // padded rows x columns a solve may hold (256 threads each
                                                         // block: the grid stays below 2^31)

enum SpectralArgError : int {
    kSpectralArgsOk = 0,
    kSpectralArgsShape,  // not 2 <= n < 2^31 (components: 1 <= n)
    kSpectralArgsNnz,    // nnz < 0
    kSpectralArgsDim,    // not 1 <= dim <= 16
    kSpectralArgsCols,   // not 1 <= p <= 32
    kSpectralArgsTol,    // tol not finite and > 0
    kSpectralArgsOuter,  // max_outer < 1
    kSpectralArgsNull,   // a null pointer that would be read or written
    kSpectralArgsAlign,  // an f64 / int64 array off an 8-byte boundary, an int32 one off a 4-byte one
    kSpectralArgsBytes,  // a byte size does not fit 63 bits, or the padded block is too large
};

inline SpectralArgError spectral_graph_args(const void* indptr, const void* indices, const void* weights,
                                            bool need_weights, int64_t n, int64_t n_min, int64_t nnz) {
    if (n < n_min || n >= kKnnMaxRows) return kSpectralArgsShape;
    if (nnz < 0) return kSpectralArgsNnz;
    if (!indptr || (nnz > 0 && (!indices || (need_weights && !weights)))) return kSpectralArgsNull;
    if (umap_misaligned(indptr, 7) || umap_misaligned(indices, 3) || (need_weights && umap_misaligned(weights, 7)))
        return kSpectralArgsAlign;
    int64_t bytes = 0;
    if (!knn_bytes(nnz, 32, 1, &bytes)) return kSpectralArgsBytes;
    return kSpectralArgsOk;
}

// karma_graph_components, everything but the graph's contents
inline SpectralArgError components_check_args(const void* indptr, const void* indices, int64_t n, int64_t nnz,
                                              const void* comp, const void* n_comp) {
    const SpectralArgError e = spectral_graph_args(indptr, indices, nullptr, false, n, 1, nnz);
    if (e != kSpectralArgsOk) return e;
    if (!comp || !n_comp) return kSpectralArgsNull;
    if (umap_misaligned(comp, 3) || umap_misaligned(n_comp, 7)) return kSpectralArgsAlign;
    return kSpectralArgsOk;
}

// karma_spectral_apply
inline SpectralArgError apply_check_args(const void* indptr, const void* indices, const void* weights, int64_t n,
                                         int64_t nnz, const void* x, int p, const void* out) {
    const SpectralArgError e = spectral_graph_args(indptr, indices, weights, true, n, 2, nnz);
    if (e != kSpectralArgsOk) return e;
    if (p < 1 || p > kSpectralColsMax) return kSpectralArgsCols;
    if (!x || !out) return kSpectralArgsNull;
    if (umap_misaligned(x, 7) || umap_misaligned(out, 7)) return kSpectralArgsAlign;
    if (n * p > kSpectralMaxCells) return kSpectralArgsBytes;
    return kSpectralArgsOk;
}

// karma_umap_spectral; vec, lam, res and comp are optional
inline SpectralArgError spectral_check_args(const void* indptr, const void* indices, const void* weights, int64_t n,
                                            int64_t nnz, int dim, double tol, int max_outer, const void* y,
                                            const void* vec, const void* lam, const void* res, const void* comp,
                                            const void* info) {
    const SpectralArgError e = spectral_graph_args(indptr, indices, weights, true, n, 2, nnz);
    if (e != kSpectralArgsOk) return e;
    if (dim < 1 || dim > kUmapDimMax) return kSpectralArgsDim;
    if (!std::isfinite(tol) || !(tol > 0.0)) return kSpectralArgsTol;
    if (max_outer < 1) return kSpectralArgsOuter;
    if (!y || !info) return kSpectralArgsNull;
    if (umap_misaligned(y, 7) || umap_misaligned(vec, 7) || umap_misaligned(lam, 7) || umap_misaligned(res, 7) ||
        umap_misaligned(info, 7) || umap_misaligned(comp, 3))
        return kSpectralArgsAlign;
    // every component is padded to whole tiles: at most n + (kSpectralTile - 1) * n rows
    if (n * kSpectralTile * (dim + kSpectralGuard) > kSpectralMaxCells) return kSpectralArgsBytes;
    return kSpectralArgsOk;
}

// a host graph's contents; weights == null (karma_graph_components): the structure alone
inline UmapArgError spectral_check_csr(const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n,
                                       int64_t nnz) {
    if (weights) return umap_check_csr(indptr, indices, weights, n, nnz);
    if (indptr[0] != 0 || indptr[n] != nnz) return kUmapArgsIndptr;
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return kUmapArgsIndptr;
    for (int64_t e = 0; e < nnz; ++e)
        if (indices[e] < 0 || indices[e] >= n) return kUmapArgsColumn;
    return kUmapArgsOk;
}

inline const char* spectral_arg_message(SpectralArgError e) {
    switch (e) {
        case kSpectralArgsShape: return "karma_spectral: need 2 <= n < 2^31 (karma_graph_components: 1 <= n)";
        case kSpectralArgsNnz: return "karma_spectral: nnz must not be negative";
        case kSpectralArgsDim: return "karma_umap_spectral: need 1 <= dim <= 16";
        case kSpectralArgsCols: return "karma_spectral_apply: need 1 <= p <= 32";
        case kSpectralArgsTol: return "karma_umap_spectral: tol must be finite and > 0";
        case kSpectralArgsOuter: return "karma_umap_spectral: need max_outer >= 1";
        case kSpectralArgsNull: return "karma_spectral: null pointer";
        case kSpectralArgsAlign:
            return "karma_spectral: f64 and int64 arrays must be 8-byte aligned, int32 arrays 4-byte aligned";
        case kSpectralArgsBytes: return "karma_spectral: a byte size overflows, or the padded block is too large";
        default: return "";
    }
}

// Rounds of karma_graph_components.  At the start of a round every tree is a
// star (the pointer jump of the round before ran to the roots), and a round
// hooks every root that has a neighbouring star with a smaller root.  Take a
// star s that is joined to another.  If s hooks, it merges.  If not, s is the
// smallest among its neighbours; a neighbour t hooks to its own smallest
// neighbour u <= s: u == s merges s now, and u < s leaves s next to a star with
// a smaller root, so s hooks in the round after.  Two rounds therefore leave
// every star of a component that still had several in a group of at least two:
// the stars at least halve (mst_args.h argues the same for Boruvka), 2 ceil(log2
// n) rounds join n vertices, and one more sees no change.
inline int components_rounds_max(int64_t n) {
    int r = 0;
    while ((int64_t(1) << r) < n) ++r;
    return 2 * r + 1;
}

}  // namespace karma
