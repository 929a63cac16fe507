// mcl_args.h — the argument checks and batch arithmetic of karma_mcl,
// karma_adj_mcl and karma_mcl_clusters: a pure host header (no HIP), shared by
// mcl.hip, mcl_clusters.cpp and mcl_args_test.cpp.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace karma {

constexpr int kMclBlock = 256;          // threads per block of the fused kernel
constexpr int kMclLanesSmall = 16;      // lanes per column, resource <= 4 (a 4 x 4 candidate square)
constexpr int kMclLanesLarge = 64;      // lanes per column, resource <= 8 (an 8 x 8 square: one wave)
constexpr int kMclFusedMaxR = 8;        // wider columns take the general path
constexpr int kMclTile = kMclBlock / kMclLanesSmall;  // columns per block of the fused kernel (16)
constexpr int kMclRMin = 2, kMclRMax = 32;
constexpr int64_t kMclCandCap = int64_t(1) << 22;     // default candidates per batch
constexpr int64_t kMclMaxN = int64_t(1) << 31;
constexpr int64_t kMclMaxSort = (int64_t(1) << 32) - 1;  // the sort's positions are u32
constexpr int kMclQueue = 4;            // fused iterations queued between reads of the chaos words

enum MclArgError : int {
    kMclArgsOk = 0,
    kMclArgsShape,      // not 1 <= n < 2^31
    kMclArgsNull,       // a null pointer that would be read or written
    kMclArgsAlign,      // an f64 / int64 array off an 8-byte boundary, a u32 / int32 one off a 4-byte one
    kMclArgsResource,   // not 2 <= resource <= 32
    kMclArgsInflation,  // not 1 < inflation <= 16
    kMclArgsCutoff,     // not 2^-40 <= cutoff <= 0.5
    kMclArgsEps,        // eps negative or NaN
    kMclArgsIter,       // max_iter < 1
    kMclArgsFlags,      // an unknown flag bit
    kMclArgsCandCap,    // cand_cap negative or >= 2^32
    kMclArgsBytes,      // a byte size does not fit 63 bits
    kMclArgsCap,        // rows and vals hold fewer than n * resource entries
    kMclArgsOff,        // off[0] != 0, decreasing, or nnz = off[n] not below 2^31
    kMclArgsNbr,        // a neighbour outside [0, n)
    kMclArgsWeight,     // a weight that is not finite and > 0
    kMclArgsDup,        // a neighbour twice in one column
    kMclArgsColptr,     // karma_mcl_clusters: colptr not a CSC of non-empty, row-sorted columns
    kMclArgsWide,       // a column's candidates exceed what one sort can take
};

inline bool mcl_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// the options every entry shares
inline MclArgError mcl_check_options(double inflation, int resource, double cutoff, double eps, int max_iter,
                                     int flags, int64_t cand_cap) {
    if (resource < kMclRMin || resource > kMclRMax) return kMclArgsResource;
    if (!(inflation > 1.0) || !(inflation <= 16.0)) return kMclArgsInflation;
    if (!(cutoff >= 0x1p-40) || !(cutoff <= 0.5)) return kMclArgsCutoff;
    if (!(eps >= 0.0)) return kMclArgsEps;
    if (max_iter < 1) return kMclArgsIter;
    if (flags & ~1) return kMclArgsFlags;
    if (cand_cap < 0 || cand_cap > kMclMaxSort) return kMclArgsCandCap;
    return kMclArgsOk;
}

// the outputs every entry shares
inline MclArgError mcl_check_outputs(int64_t n, int resource, const void* colptr, const void* rows, const void* vals,
                                     int64_t cap, const void* iterations, const void* chaos) {
    if (n < 1 || n >= kMclMaxN) return kMclArgsShape;
    if (!colptr || !rows || !vals || !iterations || !chaos) return kMclArgsNull;
    if (mcl_misaligned(colptr, 7) || mcl_misaligned(vals, 7) || mcl_misaligned(chaos, 7) || mcl_misaligned(rows, 3) ||
        mcl_misaligned(iterations, 3))
        return kMclArgsAlign;
    if (n > (INT64_MAX / 16) / kMclRMax) return kMclArgsBytes;  // n * resource * 16 bytes of matrix
    if (cap < n * resource) return kMclArgsCap;
    return kMclArgsOk;
}

// karma_mcl, everything but the graph's contents
inline MclArgError mcl_check_args(int64_t n, const void* off, const void* nbr, const void* w, double inflation,
                                  int resource, double cutoff, double eps, int max_iter, int flags, int64_t cand_cap,
                                  const void* colptr, const void* rows, const void* vals, int64_t cap,
                                  const void* iterations, const void* chaos) {
    if (n < 1 || n >= kMclMaxN) return kMclArgsShape;
    if (!off) return kMclArgsNull;  // nbr and w may be null for a graph without entries
    if (mcl_misaligned(off, 7) || mcl_misaligned(w, 7) || mcl_misaligned(nbr, 3)) return kMclArgsAlign;
    const MclArgError o = mcl_check_options(inflation, resource, cutoff, eps, max_iter, flags, cand_cap);
    if (o != kMclArgsOk) return o;
    return mcl_check_outputs(n, resource, colptr, rows, vals, cap, iterations, chaos);
}

// nnz = off[n] and the pointers that must exist with it
inline MclArgError mcl_check_nnz(int64_t first, int64_t nnz, const void* nbr, const void* w) {
    if (first != 0 || nnz < 0 || nnz >= kMclMaxN) return kMclArgsOff;
    if (nnz > 0 && (!nbr || !w)) return kMclArgsNull;
    return kMclArgsOk;
}

// a host graph's contents; seen[n] is scratch (any contents on entry)
inline MclArgError mcl_check_csr(const int64_t* off, const uint32_t* nbr, const double* w, int64_t n,
                                 std::vector<int64_t>& seen) {
    MclArgError e = mcl_check_nnz(off[0], off[n], nbr, w);
    if (e != kMclArgsOk) return e;
    for (int64_t j = 0; j < n; ++j)
        if (off[j + 1] < off[j] || off[j + 1] > off[n]) return kMclArgsOff;
    seen.assign((size_t)n, -1);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t t = off[j]; t < off[j + 1]; ++t) {
            if ((int64_t)nbr[t] >= n) return kMclArgsNbr;
            if (!(w[t] > 0.0) || !std::isfinite(w[t])) return kMclArgsWeight;
            if ((int64_t)nbr[t] == j) continue;  // entries naming j itself are ignored
            if (seen[nbr[t]] == j) return kMclArgsDup;
            seen[nbr[t]] = j;
        }
    return kMclArgsOk;
}

// karma_mcl_clusters: a CSC whose columns are non-empty and ascending by row
inline MclArgError mcl_check_matrix(int64_t n, const int64_t* colptr, const uint32_t* rows, const double* vals,
                                    const void* labels, const void* n_clusters) {
    if (n < 1 || n >= kMclMaxN) return kMclArgsShape;
    if (!colptr || !rows || !vals || !labels || !n_clusters) return kMclArgsNull;
    if (mcl_misaligned(colptr, 7) || mcl_misaligned(vals, 7) || mcl_misaligned(rows, 3) ||
        mcl_misaligned(labels, 3) || mcl_misaligned(n_clusters, 3))
        return kMclArgsAlign;
    if (colptr[0] != 0) return kMclArgsColptr;
    for (int64_t j = 0; j < n; ++j) {
        if (colptr[j + 1] <= colptr[j]) return kMclArgsColptr;
        for (int64_t t = colptr[j]; t < colptr[j + 1]; ++t) {
            if ((int64_t)rows[t] >= n) return kMclArgsNbr;
            if (t > colptr[j] && rows[t] <= rows[t - 1]) return kMclArgsColptr;
        }
    }
    return kMclArgsOk;
}

// The general path's batches: whole columns, at most cap candidates each, where
// cc[n + 1] are the columns' candidate offsets (cc[0] = 0) and cap is raised to
// the widest column's count so that a batch always holds a column.  Returns the
// batch bounds b[0] = 0 < ... < b.back() = n; *eff = the cap used.
inline std::vector<int64_t> mcl_batches(const int64_t* cc, int64_t n, int64_t cand_cap, int64_t* eff) {
    int64_t cap = cand_cap > 0 ? cand_cap : kMclCandCap;
    for (int64_t j = 0; j < n; ++j)
        if (cc[j + 1] - cc[j] > cap) cap = cc[j + 1] - cc[j];
    if (eff) *eff = cap;
    std::vector<int64_t> b{0};
    int64_t j0 = 0;
    while (j0 < n) {
        int64_t j1 = j0 + 1;  // a column always fits
        while (j1 < n && cc[j1 + 1] - cc[j0] <= cap) ++j1;
        b.push_back(j1);
        j0 = j1;
    }
    return b;
}

inline const char* mcl_arg_message(MclArgError e) {
    switch (e) {
        case kMclArgsShape: return "karma_mcl: need 1 <= n < 2^31";
        case kMclArgsNull: return "karma_mcl: null pointer";
        case kMclArgsAlign:
            return "karma_mcl: f64 and int64 arrays must be 8-byte aligned, u32 and int32 arrays 4-byte aligned";
        case kMclArgsResource: return "karma_mcl: need 2 <= resource <= 32";
        case kMclArgsInflation: return "karma_mcl: need 1 < inflation <= 16";
        case kMclArgsCutoff: return "karma_mcl: need 2^-40 <= cutoff <= 0.5";
        case kMclArgsEps: return "karma_mcl: eps must not be negative";
        case kMclArgsIter: return "karma_mcl: need max_iter >= 1";
        case kMclArgsFlags: return "karma_mcl: unknown flag";
        case kMclArgsCandCap: return "karma_mcl: need 0 <= cand_cap < 2^32";
        case kMclArgsBytes: return "karma_mcl: a byte size overflows";
        case kMclArgsCap: return "karma_mcl: rows and vals must hold n * resource entries";
        case kMclArgsOff: return "karma_mcl: off must start at 0, not decrease and end below 2^31";
        case kMclArgsNbr: return "karma_mcl: a neighbour (row) outside [0, n)";
        case kMclArgsWeight: return "karma_mcl: weights must be finite and > 0";
        case kMclArgsDup: return "karma_mcl: a neighbour twice in one column";
        case kMclArgsColptr:
            return "karma_mcl_clusters: colptr must start at 0 and every column be non-empty and ascending by row";
        case kMclArgsWide: return "karma_mcl: a column has more candidates than one sort takes (2^32 - 1)";
        default: return "";
    }
}

}  // namespace karma
