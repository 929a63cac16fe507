// umap_args.h — the argument checks of karma_umap_graph and karma_umap_layout:
// a pure host header (no HIP), shared by umap.hip and umap_args_test.cpp.
#pragma once

#include <cmath>
#include <cstdint>

#include "knn_args.h"

namespace karma {

constexpr int kUmapTile = 128;     // rows (vertices) per block of the per-row kernels
constexpr int kUmapKMin = 2;       // log2(k) must be positive
constexpr int kUmapDimMax = 16;
constexpr int64_t kUmapMaxEntries = int64_t(1) << 32;  // 2 n k candidate entries are sorted with u32 positions

enum UmapArgError : int {
    kUmapArgsOk = 0,
    kUmapArgsShape,    // not 2 <= n < 2^31
    kUmapArgsK,        // not 2 <= k <= min(n, 64)
    kUmapArgsNull,     // a null pointer that would be read or written
    kUmapArgsAlign,    // an f64 / int64 array off an 8-byte boundary, an int32 one off a 4-byte one
    kUmapArgsBytes,    // a byte size does not fit 63 bits, or 2 n k >= 2^32
    kUmapArgsCap,      // the caller's buffers hold fewer than 2 n k entries
    kUmapArgsIndex,    // a neighbour index outside [0, n)
    kUmapArgsDim,      // not 1 <= dim <= 16
    kUmapArgsEpochs,   // n_epochs < 1
    kUmapArgsRate,     // negative_sample_rate < 0
    kUmapArgsParam,    // a, b, gamma or initial_alpha not finite
    kUmapArgsNnz,      // nnz < 0
    kUmapArgsIndptr,   // indptr[0] != 0, decreasing, or not ending at nnz
    kUmapArgsColumn,   // a column outside [0, n)
    kUmapArgsWeight,   // a weight that is not finite and > 0
};

inline bool umap_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// karma_umap_graph.  sigma and rho are optional.  The lists themselves are
// looked at (umap_check_lists) only where they are host memory.
inline UmapArgError umap_graph_check_args(const void* idx, const void* dist, int64_t n, int k, const void* indptr,
                                          const void* indices, const void* weights, int64_t cap, const void* nnz,
                                          const void* sigma, const void* rho) {
    if (n < 2 || n >= kKnnMaxRows) return kUmapArgsShape;
    if (k < kUmapKMin || k > kKnnKMax || k > n) return kUmapArgsK;
    if (!idx || !dist || !indptr || !indices || !weights || !nnz) return kUmapArgsNull;
    if (umap_misaligned(dist, 7) || umap_misaligned(indptr, 7) || umap_misaligned(weights, 7) ||
        umap_misaligned(sigma, 7) || umap_misaligned(rho, 7) || umap_misaligned(nnz, 7) ||
        umap_misaligned(idx, 3) || umap_misaligned(indices, 3))
        return kUmapArgsAlign;
    int64_t bytes = 0;
    if (!knn_bytes(n, k, 32, &bytes) || 2 * n * k >= kUmapMaxEntries) return kUmapArgsBytes;
    if (cap < 2 * n * k) return kUmapArgsCap;
    return kUmapArgsOk;
}

inline UmapArgError umap_check_lists(const int32_t* idx, int64_t n, int k) {
    for (int64_t e = 0; e < n * k; ++e)
        if (idx[e] < 0 || idx[e] >= n) return kUmapArgsIndex;
    return kUmapArgsOk;
}

// karma_umap_layout, everything but the graph's contents
inline UmapArgError umap_layout_check_args(const void* indptr, const void* indices, const void* weights, int64_t n,
                                           int64_t nnz, int dim, double a, double b, int n_epochs,
                                           int negative_sample_rate, double gamma, double initial_alpha,
                                           const void* y) {
    if (n < 2 || n >= kKnnMaxRows) return kUmapArgsShape;
    if (nnz < 0) return kUmapArgsNnz;
    if (dim < 1 || dim > kUmapDimMax) return kUmapArgsDim;
    if (n_epochs < 1) return kUmapArgsEpochs;
    if (negative_sample_rate < 0) return kUmapArgsRate;
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(gamma) || !std::isfinite(initial_alpha))
        return kUmapArgsParam;
    if (!indptr || !y || (nnz > 0 && (!indices || !weights))) return kUmapArgsNull;
    if (umap_misaligned(indptr, 7) || umap_misaligned(weights, 7) || umap_misaligned(y, 7) ||
        umap_misaligned(indices, 3))
        return kUmapArgsAlign;
    int64_t bytes = 0;
    if (!knn_bytes(n, dim, 8, &bytes) || !knn_bytes(nnz, 32, 1, &bytes)) return kUmapArgsBytes;
    return kUmapArgsOk;
}

// the CSR graph's contents (host memory)
inline UmapArgError umap_check_csr(const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n,
                                   int64_t nnz) {
    if (indptr[0] != 0 || indptr[n] != nnz) return kUmapArgsIndptr;
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return kUmapArgsIndptr;
    for (int64_t e = 0; e < nnz; ++e) {
        if (indices[e] < 0 || indices[e] >= n) return kUmapArgsColumn;
        if (!(weights[e] > 0.0) || !std::isfinite(weights[e])) return kUmapArgsWeight;
    }
    return kUmapArgsOk;
}

inline const char* umap_arg_message(UmapArgError e) {
    switch (e) {
        case kUmapArgsShape: return "karma_umap: need 2 <= n < 2^31";
        case kUmapArgsK: return "karma_umap_graph: need 2 <= k <= min(n, 64)";
        case kUmapArgsNull: return "karma_umap: null pointer";
        case kUmapArgsAlign:
            return "karma_umap: f64 and int64 arrays must be 8-byte aligned, int32 arrays 4-byte aligned";
        case kUmapArgsBytes: return "karma_umap: a byte size overflows (the graph needs 2 n k < 2^32)";
        case kUmapArgsCap: return "karma_umap_graph: indices and weights must hold 2 n k entries";
        case kUmapArgsIndex: return "karma_umap_graph: a neighbour index outside [0, n)";
        case kUmapArgsDim: return "karma_umap_layout: need 1 <= dim <= 16";
        case kUmapArgsEpochs: return "karma_umap_layout: need n_epochs >= 1";
        case kUmapArgsRate: return "karma_umap_layout: negative_sample_rate must not be negative";
        case kUmapArgsParam: return "karma_umap_layout: a, b, gamma and initial_alpha must be finite";
        case kUmapArgsNnz: return "karma_umap_layout: nnz must not be negative";
        case kUmapArgsIndptr: return "karma_umap_layout: indptr must start at 0, not decrease and end at nnz";
        case kUmapArgsColumn: return "karma_umap_layout: a column outside [0, n)";
        case kUmapArgsWeight: return "karma_umap_layout: weights must be finite and > 0";
        default: return "";
    }
}

}  // namespace karma
