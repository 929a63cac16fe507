// knn_args.h — karma_knn_rows' tile constants and argument checks: a pure host
// header (no HIP), shared by knn.hip and knn_args_test.cpp.
#pragma once

#include <cstdint>

namespace karma {

// The kernel's tile.  A block of kKnnThreads threads (a 16 x 16 grid) owns
// kKnnQ query rows and walks the candidates kKnnC rows at a time; both tiles
// are staged in LDS kKnnPanel columns at a time; a thread accumulates an
// 8 x 8 tile of pairs.  Each query row keeps a sorted list of k <= kKnnKMax
// entries in LDS.
constexpr int kKnnThreads = 256;
constexpr int kKnnQ = 128;
constexpr int kKnnC = 128;
constexpr int kKnnPanel = 16;
constexpr int kKnnKMax = 64;

constexpr int64_t kKnnMaxRows = int64_t(1) << 31;  // indices are int32

enum KnnArgError : int {
    kKnnArgsOk = 0,
    kKnnArgsShape,   // n < 0, m < 0, or n >= 2^31
    kKnnArgsStride,  // ld < m
    kKnnArgsRange,   // not 0 <= row_lo <= row_hi <= n
    kKnnArgsK,       // not 1 <= k <= min(n, kKnnKMax) (with rows to answer)
    kKnnArgsNull,    // a null pointer with rows to answer
    kKnnArgsAlign,   // x or dist off an 8-byte boundary, idx off a 4-byte one
    kKnnArgsBytes,   // a byte size does not fit 63 bits
};

// a * b * c in 63 bits (all >= 0); false when it does not fit
inline bool knn_bytes(int64_t a, int64_t b, int64_t c, int64_t* out) {
    const int64_t lim = INT64_MAX;
    if (a && b > lim / a) return false;
    const int64_t ab = a * b;
    if (ab && c > lim / ab) return false;
    *out = ab * c;
    return true;
}

// Nothing is read or written when n == 0 or the range is empty: pointers and k
// are then not looked at.
inline KnnArgError knn_check_args(const void* x, int64_t n, int64_t m, int64_t ld, int64_t row_lo, int64_t row_hi,
                                  int k, const void* idx, const void* dist) {
    if (n < 0 || m < 0 || n >= kKnnMaxRows) return kKnnArgsShape;
    if (ld < m) return kKnnArgsStride;
    if (row_lo < 0 || row_hi < row_lo || row_hi > n) return kKnnArgsRange;
    if (n == 0 || row_lo == row_hi) return kKnnArgsOk;
    if (k < 1 || k > kKnnKMax || k > n) return kKnnArgsK;
    if (!idx || !dist || (m > 0 && !x)) return kKnnArgsNull;
    if ((reinterpret_cast<uintptr_t>(x) & 7) || (reinterpret_cast<uintptr_t>(dist) & 7) ||
        (reinterpret_cast<uintptr_t>(idx) & 3))
        return kKnnArgsAlign;
    int64_t b = 0;
    if (!knn_bytes(n, ld, 8, &b) || !knn_bytes(row_hi - row_lo, k, 8, &b)) return kKnnArgsBytes;
    return kKnnArgsOk;
}

inline const char* knn_arg_message(KnnArgError e) {
    switch (e) {
        case kKnnArgsShape: return "karma_knn_rows: n and m must not be negative, and n < 2^31";
        case kKnnArgsStride: return "karma_knn_rows: ld must be at least m";
        case kKnnArgsRange: return "karma_knn_rows: need 0 <= row_lo <= row_hi <= n";
        case kKnnArgsK: return "karma_knn_rows: need 1 <= k <= min(n, 64)";
        case kKnnArgsNull: return "karma_knn_rows: null pointer";
        case kKnnArgsAlign: return "karma_knn_rows: x and dist must be 8-byte aligned, idx 4-byte aligned";
        case kKnnArgsBytes: return "karma_knn_rows: a byte size overflows";
        default: return "";
    }
}

}  // namespace karma
