// Host unit test of sets_ctrl.h (no GPU): every offset of the records job's
// control block against the arithmetic the job's code spelled out before the
// layout had a name, and no two regions overlapping.  Built by `make -C
// karma_amd/csrc sets_ctrl_test`, run by tests/test_sets_ctrl_cpu.py.  Exit
// status 0 = every case passed.
#include <cstdio>
#include <initializer_list>

#include "sets_ctrl.h"

using namespace karma;

namespace {
int g_bad = 0, g_cases = 0;

#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++g_bad;                                               \
        }                                                          \
    } while (0)

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

void check(int64_t B, int64_t n_split, int64_t n_pblk) {
    const int bad0 = g_bad;
    const CtrlLayout L(B, n_split, n_pblk);
    ++g_cases;
    // SetsJob::setup: flags = cb, counters = cb + 2, n_per = cb + 6, dst = n_per + (B + 1),
    // ovf = dst + (B + 1), split_loc = dst + (B + 1) + ceil_div(B, 8)
    EXPECT(L.flags == 0);
    EXPECT(L.counters == 2);
    EXPECT(L.n_per == 6);
    EXPECT(L.dst == 6 + (B + 1));
    EXPECT(L.ovf == 6 + 2 * (B + 1));
    EXPECT(L.split_loc == 6 + 2 * (B + 1) + ceil_div(B, 8));
    // ctrl_words = 6 + 2 (B + 1) + ceil_div(B, 8) + n_split; blk_items = cb + ctrl_words;
    // lb = cb + ctrl_words + 2 n_pblk; the memset's size ctrl_words + 2 n_pblk + B
    const int64_t ctrl_words = 6 + 2 * (B + 1) + ceil_div(B, 8) + n_split;
    EXPECT(L.readback == ctrl_words);
    EXPECT(L.blk_items == ctrl_words);
    EXPECT(L.lb == ctrl_words + 2 * n_pblk);
    EXPECT(L.total == ctrl_words + 2 * n_pblk + B);
    // SetsJob::finish: U = hctrl[6 + (B + 1) + B]
    EXPECT(L.list_len == 6 + (B + 1) + B);
    // regions [start, end) in words, in order, none overlapping, the last ending at total;
    // the flags and counters in use fit theirs, the overflow bytes theirs
    const int64_t at[] = {L.flags, L.counters, L.n_per, L.dst, L.ovf, L.split_loc, L.blk_items, L.lb, L.total};
    const int64_t len[] = {(kCtrlFlags * 4 + 7) / 8, (kCtrlCounters * 4 + 7) / 8, B + 1, B + 1, ceil_div(B, 8),
                           n_split,                  2 * n_pblk,                  B};
    for (int r = 0; r < 8; ++r) EXPECT(at[r] >= 0 && at[r] + len[r] <= at[r + 1]);
    EXPECT(L.ovf * 8 + B <= L.split_loc * 8);
    EXPECT(L.list_len >= L.dst && L.list_len < L.ovf);
    EXPECT(L.readback <= L.total);
    EXPECT(CtrlLayout::small_words * 8 >= CtrlLayout::counters * 8 + (kCtrBigReads + 1) * 4);
    if (g_bad != bad0)
        std::printf("  at B %lld n_split %lld n_pblk %lld\n", (long long)B, (long long)n_split, (long long)n_pblk);
}
}  // namespace

int main() {
    // the enumerators are the indices the kernels and the host used as bare integers
    EXPECT(kFlagOrder == 0 && kFlagContigRange == 1 && kFlagPairCap == 2 && kFlagPartition == 3);
    EXPECT(kCtrBigReads == 0 && kCtrCodeFlushes == 1 && kCtrPairFlushes == 2 && kCtrRelabel == 3 && kCtrVote == 4);
    for (int64_t B : {1, 7, 8, 9, 196, 2048})  // 7, 8, 9: around one word of overflow bytes; 196: config 3
        for (int64_t n_split : {0, 9})
            for (int64_t n_pblk : {1, 5}) check(B, n_split, n_pblk);
    std::printf("%s (%d cases, %d failures)\n", g_bad ? "FAILED" : "ok", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
