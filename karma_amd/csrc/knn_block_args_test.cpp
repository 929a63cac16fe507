// knn_block_args_test.cpp — the blockwise neighbour entries' argument checks
// and candidate-split arithmetic (knn_block_args.h) on the host, built with
// AddressSanitizer + UBSan (make knn_block_args_test;
// tests/test_knn_block_args_cpu.py).  No GPU code.
#include <cstdio>
#include <vector>

#include "knn_block_args.h"

using namespace karma;

static int g_cases = 0, g_failed = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        ++g_cases;                                                       \
        if (!(cond)) {                                                   \
            ++g_failed;                                                  \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                                \
    } while (0)

int main() {
    static_assert(kKnnMaxIndex == 2147483647, "indices are int32 and INT32_MAX marks an empty slot");
    static_assert(kKnnSplitMax == 32 && kKnnSplitMax + 1 <= 64, "a wave's lanes hold the carried and the partial lists");
    static_assert(kKnnKMax == 64, "knn_block_arg_message names the limit");

    std::vector<double> qs(64), cs(64);
    std::vector<uint64_t> ks(64);
    std::vector<int32_t> is(64);
    const double *q = qs.data(), *c = cs.data();
    const uint64_t* k = ks.data();
    const int32_t* i = is.data();
    const char* qb = reinterpret_cast<const char*>(q);
    const char* kb = reinterpret_cast<const char*>(k);
    const char* ib = reinterpret_cast<const char*>(i);

    // karma_knn_block: (q, nq, ldq, c, nc, ldc, m, cand_base, k, keys, idx, cand_split)
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockOk);
    EXPECT(knn_block_check_args(q, 8, 7, c, 5, 9, 4, 100, 64, k, i, 1000) == kKnnBlockOk);  // strides, k > nc, large S
    EXPECT(knn_block_check_args(nullptr, 8, 0, nullptr, 5, 0, 0, 0, 1, k, i, 1) == kKnnBlockOk);  // no columns
    EXPECT(knn_block_check_args(nullptr, 8, 4, nullptr, 0, 4, 4, 0, 1, k, i, 1) == kKnnBlockOk);  // no candidates
    // nothing to do: neither pointers nor k are looked at
    EXPECT(knn_block_check_args(nullptr, 0, 4, nullptr, 5, 4, 4, 0, 0, nullptr, nullptr, -1) == kKnnBlockOk);
    // shape
    EXPECT(knn_block_check_args(q, -1, 4, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockShape);
    EXPECT(knn_block_check_args(q, 8, 4, c, -1, 4, 4, 0, 3, k, i, 0) == kKnnBlockShape);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, -1, 0, 3, k, i, 0) == kKnnBlockShape);
    EXPECT(knn_block_check_args(q, kKnnMaxRows, 1, c, 5, 1, 1, 0, 3, k, i, 0) == kKnnBlockShape);
    EXPECT(knn_block_check_args(q, kKnnMaxRows - 1, 1, c, 5, 1, 1, 0, 3, k, i, 0) == kKnnBlockOk);
    // strides
    EXPECT(knn_block_check_args(q, 8, 3, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockStride);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 3, 4, 0, 3, k, i, 0) == kKnnBlockStride);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, -4, 4, 0, 3, k, i, 0) == kKnnBlockStride);
    // base and index overflow: the last index may be 2^31 - 2
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, -1, 3, k, i, 0) == kKnnBlockBase);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, kKnnMaxIndex - 5, 3, k, i, 0) == kKnnBlockOk);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, kKnnMaxIndex - 4, 3, k, i, 0) == kKnnBlockBase);
    EXPECT(knn_block_check_args(q, 8, 4, c, 0, 4, 4, kKnnMaxIndex, 3, k, i, 0) == kKnnBlockOk);
    EXPECT(knn_block_check_args(q, 8, 4, c, 0, 4, 4, kKnnMaxIndex + 1, 3, k, i, 0) == kKnnBlockBase);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, INT64_MAX, 3, k, i, 0) == kKnnBlockBase);
    EXPECT(knn_block_check_args(q, 8, 1, c, INT64_MAX, 1, 1, 1, 3, k, i, 0) == kKnnBlockBase);  // no wrap in base + nc
    // k
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 0, k, i, 0) == kKnnBlockK);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, -1, k, i, 0) == kKnnBlockK);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, kKnnKMax + 1, k, i, 0) == kKnnBlockK);
    // split
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, k, i, -1) == kKnnBlockSplit);
    // null pointers
    EXPECT(knn_block_check_args(nullptr, 8, 4, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockNull);
    EXPECT(knn_block_check_args(q, 8, 4, nullptr, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockNull);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, nullptr, i, 0) == kKnnBlockNull);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, k, nullptr, 0) == kKnnBlockNull);
    EXPECT(knn_block_check_args(nullptr, 8, 4, nullptr, 0, 4, 4, 0, 3, nullptr, i, 1) == kKnnBlockNull);  // the state always
    // alignment
    EXPECT(knn_block_check_args(qb + 4, 7, 4, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockAlign);
    EXPECT(knn_block_check_args(q, 8, 4, reinterpret_cast<const char*>(c) + 4, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockAlign);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, kb + 4, i, 0) == kKnnBlockAlign);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, k, ib + 2, 0) == kKnnBlockAlign);
    EXPECT(knn_block_check_args(q, 8, 4, c, 5, 4, 4, 0, 3, k, i + 1, 0) == kKnnBlockOk);  // idx owes 4 bytes only
    // byte sizes
    const int64_t big = int64_t(1) << 40;
    EXPECT(knn_block_check_args(q, int64_t(1) << 20, big, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockBytes);  // 2^63
    EXPECT(knn_block_check_args(q, (int64_t(1) << 20) - 1, big, c, 5, 4, 4, 0, 3, k, i, 0) == kKnnBlockOk);
    EXPECT(knn_block_check_args(q, 8, 4, c, int64_t(1) << 20, big, 4, 0, 3, k, i, 0) == kKnnBlockBytes);
    // the first failing check names the error
    EXPECT(knn_block_check_args(nullptr, 8, 3, nullptr, 5, 4, 4, -1, 0, nullptr, nullptr, -1) == kKnnBlockStride);
    EXPECT(knn_block_check_args(nullptr, 8, 4, nullptr, 5, 4, 4, -1, 0, nullptr, nullptr, -1) == kKnnBlockBase);
    EXPECT(knn_block_check_args(nullptr, 8, 4, nullptr, 5, 4, 4, 0, 0, nullptr, nullptr, -1) == kKnnBlockK);
    EXPECT(knn_block_check_args(nullptr, 8, 4, nullptr, 5, 4, 4, 0, 1, nullptr, nullptr, -1) == kKnnBlockSplit);

    // karma_knn_merge / karma_knn_finish: (keys, idx, second keys or dist, second idx, nq, k)
    EXPECT(knn_lists_check_args(k, i, k + 32, i + 32, 4, 8) == kKnnBlockOk);
    EXPECT(knn_lists_check_args(nullptr, nullptr, nullptr, nullptr, 0, 0) == kKnnBlockOk);
    EXPECT(knn_lists_check_args(k, i, k, i, -1, 8) == kKnnBlockShape);
    EXPECT(knn_lists_check_args(k, i, k, i, kKnnMaxRows, 8) == kKnnBlockShape);
    EXPECT(knn_lists_check_args(k, i, k, i, 4, 0) == kKnnBlockK);
    EXPECT(knn_lists_check_args(k, i, k, i, 4, 65) == kKnnBlockK);
    EXPECT(knn_lists_check_args(nullptr, i, k, i, 4, 8) == kKnnBlockNull);
    EXPECT(knn_lists_check_args(k, nullptr, k, i, 4, 8) == kKnnBlockNull);
    EXPECT(knn_lists_check_args(k, i, nullptr, i, 4, 8) == kKnnBlockNull);
    EXPECT(knn_lists_check_args(k, i, k, nullptr, 4, 8) == kKnnBlockNull);
    EXPECT(knn_lists_check_args(kb + 4, i, k, i, 4, 8) == kKnnBlockAlign);
    EXPECT(knn_lists_check_args(k, ib + 2, k, i, 4, 8) == kKnnBlockAlign);
    EXPECT(knn_lists_check_args(k, i, kb + 4, i, 4, 8) == kKnnBlockAlign);
    EXPECT(knn_lists_check_args(k, i, k, ib + 1, 4, 8) == kKnnBlockAlign);

    for (int e = kKnnBlockShape; e <= kKnnBlockBytes; ++e) EXPECT(knn_block_arg_message((KnnBlockArgError)e)[0] != 0);
    EXPECT(knn_block_arg_message(kKnnBlockOk)[0] == 0);

    // the split: clamped to the tiles and to kKnnSplitMax, at least 1
    EXPECT(knn_cand_tiles(0) == 0 && knn_cand_tiles(1) == 1 && knn_cand_tiles(kKnnC) == 1 && knn_cand_tiles(kKnnC + 1) == 2);
    EXPECT(knn_split_resolve(100, 3 * kKnnC, 1, 0) == 1);
    EXPECT(knn_split_resolve(100, 3 * kKnnC, 2, 0) == 2);
    EXPECT(knn_split_resolve(100, 3 * kKnnC - 1, 7, 0) == 3);
    EXPECT(knn_split_resolve(100, 9 * kKnnC - 5, 7, 0) == 7);
    EXPECT(knn_split_resolve(100, 9 * kKnnC - 5, 1000, 0) == 9);
    EXPECT(knn_split_resolve(100, 1000 * kKnnC, 1000, 0) == kKnnSplitMax);
    EXPECT(knn_split_resolve(100, 0, 5, 0) == 1);
    EXPECT(knn_split_resolve(100, 1, 0, 0) == 1);
    // auto: the largest S whose blocks fit the capacity
    EXPECT(knn_split_resolve(300, 20000, 0, 512) == kKnnSplitMax);  // 3 query blocks: 170 would fit
    EXPECT(knn_split_resolve(25000, 200000, 0, 512) == 2);          // 196 query blocks
    EXPECT(knn_split_resolve(25000, 200000, 0, 256) == 1);
    EXPECT(knn_split_resolve(100000, 200000, 0, 512) == 1);         // more than one round already
    EXPECT(knn_split_resolve(300, 2 * kKnnC, 0, 512) == 2);
    EXPECT(knn_split_resolve(0, 2 * kKnnC, 0, 512) == 1);
    // slices: contiguous whole tiles that cover [0, tiles), none empty when S <= tiles, sizes within one
    for (int64_t tiles : {1, 2, 3, 9, 157, 1563})
        for (int S = 1; S <= kKnnSplitMax && S <= tiles; ++S) {
            int64_t lo = INT64_MAX, hi = 0;
            EXPECT(knn_slice_begin(tiles, S, 0) == 0 && knn_slice_begin(tiles, S, S) == tiles);
            for (int s = 0; s < S; ++s) {
                const int64_t n = knn_slice_begin(tiles, S, s + 1) - knn_slice_begin(tiles, S, s);
                lo = n < lo ? n : lo;
                hi = n > hi ? n : hi;
            }
            EXPECT(lo >= 1 && hi - lo <= 1);
        }

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
