// mst_args.h — karma_mreach_mst's argument checks and round bound: a pure host
// header (no HIP), shared by mst.hip and mst_args_test.cpp.  The tile is
// karma_knn_rows' (knn_args.h).
#pragma once

#include <cstdint>

#include "knn_args.h"

namespace karma {

constexpr int kMstSplitMax = 32;  // slices of the candidate tiles that run side by side

enum MstArgError : int {
    kMstArgsOk = 0,
    kMstArgsShape,    // n < 1, m < 0, or n >= 2^31
    kMstArgsStride,   // ld < m
    kMstArgsSamples,  // not 1 <= min_samples <= min(n, kKnnKMax)
    kMstArgsNull,     // a null pointer that would be read or written
    kMstArgsAlign,    // x, w or core off an 8-byte boundary, a or b off a 4-byte one
    kMstArgsBytes,    // a byte size does not fit 63 bits
};

inline bool mst_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// a, b and w are looked at only when there is an edge to write (n > 1); x only when m > 0
inline MstArgError mst_check_args(const void* x, int64_t n, int64_t m, int64_t ld, int min_samples, const void* a,
                                  const void* b, const void* w, const void* core) {
    if (n < 1 || m < 0 || n >= kKnnMaxRows) return kMstArgsShape;
    if (ld < m) return kMstArgsStride;
    if (min_samples < 1 || min_samples > kKnnKMax || min_samples > n) return kMstArgsSamples;
    if (!core || (m > 0 && !x) || (n > 1 && (!a || !b || !w))) return kMstArgsNull;
    if (mst_misaligned(x, 7) || mst_misaligned(core, 7) || mst_misaligned(w, 7) || mst_misaligned(a, 3) ||
        mst_misaligned(b, 3))
        return kMstArgsAlign;
    int64_t bytes = 0;
    if (!knn_bytes(n, ld, 8, &bytes) || !knn_bytes(n, min_samples, 8, &bytes) || !knn_bytes(n, kMstSplitMax, 8, &bytes))
        return kMstArgsBytes;
    return kMstArgsOk;
}

inline const char* mst_arg_message(MstArgError e) {
    switch (e) {
        case kMstArgsShape: return "karma_mreach_mst: need 1 <= n < 2^31 and m >= 0";
        case kMstArgsStride: return "karma_mreach_mst: ld must be at least m";
        case kMstArgsSamples: return "karma_mreach_mst: need 1 <= min_samples <= min(n, 64)";
        case kMstArgsNull: return "karma_mreach_mst: null pointer";
        case kMstArgsAlign: return "karma_mreach_mst: x, w and core must be 8-byte aligned, a and b 4-byte aligned";
        case kMstArgsBytes: return "karma_mreach_mst: a byte size overflows";
        default: return "";
    }
}

// Boruvka rounds at least halve the number of components: ceil(log2 n) rounds
// join n rows (0 for n == 1).
inline int mst_rounds_max(int64_t n) {
    int r = 0;
    while ((int64_t(1) << r) < n) ++r;
    return r;
}

// Slices of the candidate tiles a round runs with: the largest S <=
// kMstSplitMax whose ceil(n / kKnnQ) * S blocks fit in `capacity` (blocks
// resident on the device at once), at most the number of tiles, at least 1.
inline int mst_split(int64_t n, int64_t capacity) {
    const int64_t tiles = (n + kKnnC - 1) / kKnnC, qb = (n + kKnnQ - 1) / kKnnQ;
    int64_t s = qb > 0 ? capacity / qb : 1;
    if (s > kMstSplitMax) s = kMstSplitMax;
    if (s > tiles) s = tiles;
    return s < 1 ? 1 : (int)s;
}

}  // namespace karma
