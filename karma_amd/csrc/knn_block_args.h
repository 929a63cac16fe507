// knn_block_args.h — argument checks of the blockwise neighbour entries
// (karma_knn_block, karma_knn_merge, karma_knn_finish, karma_knn_block_split)
// and the candidate split's arithmetic: a pure host header (no HIP), shared by
// knn_block.hip and knn_block_args_test.cpp.
#pragma once

#include <cstdint>

#include "knn_args.h"

namespace karma {

constexpr int64_t kKnnMaxIndex = (int64_t(1) << 31) - 1;  // cand_base + nc may reach it: indices stay below INT32_MAX
constexpr int kKnnSplitMax = 32;                          // partial lists a merge folds (plus the carried one: a wave's lanes)

enum KnnBlockArgError : int {
    kKnnBlockOk = 0,
    kKnnBlockShape,   // nq, nc or m negative, or nq >= 2^31
    kKnnBlockStride,  // ldq < m or ldc < m
    kKnnBlockBase,    // cand_base < 0 or cand_base + nc > 2^31 - 1
    kKnnBlockK,       // not 1 <= k <= kKnnKMax
    kKnnBlockSplit,   // cand_split < 0
    kKnnBlockNull,    // a null pointer that would be read or written
    kKnnBlockAlign,   // a matrix or keys off an 8-byte boundary, idx off a 4-byte one
    kKnnBlockBytes,   // a byte size does not fit 63 bits
};

inline bool knn_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// karma_knn_block.  nq == 0: nothing is read or written, pointers and k are
// not looked at.  k may exceed nc.  c is read only when nc > 0 and m > 0, q
// only when it has rows and m > 0; the state is looked at whenever nq > 0.
inline KnnBlockArgError knn_block_check_args(const void* q, int64_t nq, int64_t ldq, const void* c, int64_t nc,
                                             int64_t ldc, int64_t m, int64_t cand_base, int k, const void* keys,
                                             const void* idx, int cand_split) {
    if (nq < 0 || nc < 0 || m < 0 || nq >= kKnnMaxRows) return kKnnBlockShape;
    if (ldq < m || ldc < m) return kKnnBlockStride;
    if (cand_base < 0 || cand_base > kKnnMaxIndex || nc > kKnnMaxIndex - cand_base) return kKnnBlockBase;
    if (nq == 0) return kKnnBlockOk;
    if (k < 1 || k > kKnnKMax) return kKnnBlockK;
    if (cand_split < 0) return kKnnBlockSplit;
    if (!keys || !idx || (m > 0 && nc > 0 && (!q || !c))) return kKnnBlockNull;
    if (knn_misaligned(q, 7) || knn_misaligned(c, 7) || knn_misaligned(keys, 7) || knn_misaligned(idx, 3))
        return kKnnBlockAlign;
    int64_t b = 0;
    if (!knn_bytes(nq, ldq, 8, &b) || !knn_bytes(nc, ldc, 8, &b) || !knn_bytes(nq, k, 8, &b)) return kKnnBlockBytes;
    return kKnnBlockOk;
}

// karma_knn_merge (b_*: the second list) and karma_knn_finish (b_keys: out_dist,
// b_idx: out_idx): two pairs of (8-byte, 4-byte) arrays of nq x k.
inline KnnBlockArgError knn_lists_check_args(const void* keys, const void* idx, const void* b_keys, const void* b_idx,
                                             int64_t nq, int k) {
    if (nq < 0 || nq >= kKnnMaxRows) return kKnnBlockShape;
    if (nq == 0) return kKnnBlockOk;
    if (k < 1 || k > kKnnKMax) return kKnnBlockK;
    if (!keys || !idx || !b_keys || !b_idx) return kKnnBlockNull;
    if (knn_misaligned(keys, 7) || knn_misaligned(b_keys, 7) || knn_misaligned(idx, 3) || knn_misaligned(b_idx, 3))
        return kKnnBlockAlign;
    return kKnnBlockOk;
}

inline const char* knn_block_arg_message(KnnBlockArgError e) {
    switch (e) {
        case kKnnBlockShape: return "nq, nc and m must not be negative, and nq < 2^31";
        case kKnnBlockStride: return "ldq and ldc must be at least m";
        case kKnnBlockBase: return "need 0 <= cand_base and cand_base + nc <= 2^31 - 1";
        case kKnnBlockK: return "need 1 <= k <= 64";
        case kKnnBlockSplit: return "cand_split must not be negative";
        case kKnnBlockNull: return "null pointer";
        case kKnnBlockAlign: return "matrices, keys and dist must be 8-byte aligned, idx 4-byte aligned";
        case kKnnBlockBytes: return "a byte size overflows";
        default: return "";
    }
}

// Candidate tiles of a block of nc rows.
inline int64_t knn_cand_tiles(int64_t nc) { return (nc + kKnnC - 1) / kKnnC; }

// The split a call runs with.  cand_split >= 1 is clamped to the number of
// candidate tiles and to kKnnSplitMax; 0 (auto) is the largest S <= kKnnSplitMax
// whose ceil(nq / kKnnQ) * S blocks fit in `capacity` (the blocks resident on the
// device at once), clamped the same way.  At least 1.
inline int knn_split_resolve(int64_t nq, int64_t nc, int cand_split, int64_t capacity) {
    const int64_t tiles = knn_cand_tiles(nc);
    int64_t s = cand_split;
    if (cand_split == 0) {
        const int64_t qb = (nq + kKnnQ - 1) / kKnnQ;
        s = qb > 0 ? capacity / qb : 1;
    }
    if (s > kKnnSplitMax) s = kKnnSplitMax;
    if (s > tiles) s = tiles;
    return s < 1 ? 1 : (int)s;
}

// Slice s of S walks the candidate tiles [knn_slice_begin(tiles, S, s),
// knn_slice_begin(tiles, S, s + 1)): contiguous, whole tiles, none empty when
// S <= tiles, sizes differing by at most one.
constexpr int64_t knn_slice_begin(int64_t tiles, int S, int s) { return tiles * s / S; }

}  // namespace karma
