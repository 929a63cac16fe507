// flag_args_test.cpp — karma_records_flag's argument and overlap checks
// (flag_args.h) on the host, built with AddressSanitizer + UBSan
// (make flag_args_test; tests/test_flag_records_device_cpu.py).  No GPU code.
#include <cstdio>
#include <vector>

#include "flag_args.h"

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

// bytes [a, a + na) and [b, b + nb) share one, decided byte by byte
static bool overlap_slow(uint64_t a, uint64_t na, uint64_t b, uint64_t nb) {
    for (uint64_t x = a; x < a + na; ++x)
        if (x >= b && x < b + nb) return true;
    return false;
}

int main() {
    static_assert(kFlagPer * 4 == 16, "a lane stores one 16-byte vector of words");
    static_assert(kFlagWave == 64 * kFlagPer && kFlagRound == kFlagThreads * kFlagPer, "tile");
    static_assert(kFlagTile == kFlagRound * kFlagRounds && kFlagTile % kFlagWave == 0, "tile");

    // the overlap predicate against the byte-by-byte definition, around every relative position
    for (uint64_t na : {0, 1, 8, 24})
        for (uint64_t nb : {0, 1, 4, 12})
            for (uint64_t a = 64; a < 64 + 40; ++a)
                for (uint64_t b = 64; b < 64 + 40; ++b)
                    EXPECT(flag_ranges_overlap((uintptr_t)a, na, (uintptr_t)b, nb) == overlap_slow(a, na, b, nb));
    // ranges at the top of the address space do not wrap
    EXPECT(!flag_ranges_overlap(~(uintptr_t)0 - 15, 8, ~(uintptr_t)0 - 7, 8));
    EXPECT(flag_ranges_overlap(~(uintptr_t)0 - 15, 9, ~(uintptr_t)0 - 7, 8));

    std::vector<uint32_t> buf(64);
    uint32_t* p = buf.data();
    const int n = 8;  // 16 words of records, 8 of output
    EXPECT(flag_check_args(p, n, 0, 0, p + 16, 0) == kFlagArgsOk);       // touching
    EXPECT(flag_check_args(p, n, 1, 1, p + 16, 1) == kFlagArgsOk);
    EXPECT(flag_check_args(p, n, 0, 0, p + 15, 0) == kFlagArgsOverlap);  // out starts in the last record
    EXPECT(flag_check_args(p + 8, n, 0, 1, p, 1) == kFlagArgsOk);        // out ends where the records start
    EXPECT(flag_check_args(p + 7, n, 0, 1, p, 1) == kFlagArgsOverlap);
    EXPECT(flag_check_args(p, n, 0, 0, p, 0) == kFlagArgsOverlap);       // in place
    EXPECT(flag_check_args(p, n, 0, 1, p, 0) == kFlagArgsOk);            // two address spaces: never compared
    EXPECT(flag_check_args(p, n, 0, 0, p, 1) == kFlagArgsOk);
    EXPECT(flag_check_args(nullptr, 0, 0, 0, nullptr, 0) == kFlagArgsOk);  // nothing to do
    EXPECT(flag_check_args(p, 0, 1, 1, p, 1) == kFlagArgsOk);
    EXPECT(flag_check_args(nullptr, 1, 0, 0, p, 0) == kFlagArgsNull);
    EXPECT(flag_check_args(p, 1, 0, 0, nullptr, 0) == kFlagArgsNull);
    EXPECT(flag_check_args(p, -1, 0, 0, p + 32, 0) == kFlagArgsNull);
    EXPECT(flag_check_args(p, n, 2, 0, p + 32, 0) == kFlagArgsFormat);   // KARMA_REC_FLAGGED is no input format
    EXPECT(flag_check_args(p, n, -1, 0, p + 32, 0) == kFlagArgsFormat);
    EXPECT(flag_check_args(p, kFlagMaxSorted, 0, 1, p + 32, 0) == kFlagArgsTooMany);
    EXPECT(flag_check_args(p, kFlagMaxSorted - 1, 0, 1, p + 32, 0) == kFlagArgsOk);
    EXPECT(flag_check_args(p, kFlagMaxUnsorted, 1, 1, p + 32, 0) == kFlagArgsTooMany);
    EXPECT(flag_check_args(p, kFlagMaxUnsorted - 1, 1, 1, p + 32, 0) == kFlagArgsOk);
    EXPECT(flag_check_args(p, kFlagMaxUnsorted, 0, 1, p + 32, 0) == kFlagArgsOk);
    const char* c = reinterpret_cast<const char*>(p);
    EXPECT(flag_check_args(c + 2, n, 0, 0, p + 32, 0) == kFlagArgsAlign);
    EXPECT(flag_check_args(p, n, 0, 0, c + 129, 0) == kFlagArgsAlign);
    EXPECT(flag_check_args(c + 4, n, 0, 0, c + 140, 0) == kFlagArgsOk);  // 4-byte alignment is all a caller owes
    for (int e = kFlagArgsNull; e <= kFlagArgsOverlap; ++e) EXPECT(flag_arg_message((FlagArgError)e)[0] != 0);

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
