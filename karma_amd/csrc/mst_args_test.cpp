// mst_args_test.cpp — karma_mreach_mst's argument checks, round bound and
// candidate split (mst_args.h) on the host, built with AddressSanitizer + UBSan
// (make mst_args_test; tests/test_mst_args_cpu.py).  No GPU code.
#include <cstdio>
#include <vector>

#include "mst_args.h"

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
    static_assert(kKnnKMax == 64, "mst_arg_message names the limit");
    static_assert(kKnnQ == kKnnC, "one id range per tile serves queries and candidates");

    std::vector<double> xs(64), ws(64), cs(64);
    std::vector<int32_t> as(64), bs(64);
    const double* x = xs.data();
    double *w = ws.data(), *c = cs.data();
    int32_t *a = as.data(), *b = bs.data();

    EXPECT(mst_check_args(x, 8, 4, 4, 3, a, b, w, c) == kMstArgsOk);
    EXPECT(mst_check_args(x, 8, 4, 7, 8, a, b, w, c) == kMstArgsOk);        // ld > m, min_samples == n
    EXPECT(mst_check_args(nullptr, 8, 0, 0, 1, a, b, w, c) == kMstArgsOk);  // no columns: every d2 is +0
    EXPECT(mst_check_args(x, 1, 4, 4, 1, nullptr, nullptr, nullptr, c) == kMstArgsOk);  // one row: no edge
    // shape
    EXPECT(mst_check_args(x, 0, 4, 4, 1, a, b, w, c) == kMstArgsShape);
    EXPECT(mst_check_args(x, -1, 4, 4, 1, a, b, w, c) == kMstArgsShape);
    EXPECT(mst_check_args(x, 8, -1, 4, 1, a, b, w, c) == kMstArgsShape);
    EXPECT(mst_check_args(x, kKnnMaxRows, 1, 1, 1, a, b, w, c) == kMstArgsShape);
    EXPECT(mst_check_args(x, kKnnMaxRows - 1, 1, 1, 1, a, b, w, c) == kMstArgsOk);
    // stride
    EXPECT(mst_check_args(x, 8, 4, 3, 1, a, b, w, c) == kMstArgsStride);
    EXPECT(mst_check_args(x, 8, 4, -4, 1, a, b, w, c) == kMstArgsStride);
    // min_samples
    EXPECT(mst_check_args(x, 8, 4, 4, 0, a, b, w, c) == kMstArgsSamples);
    EXPECT(mst_check_args(x, 8, 4, 4, -1, a, b, w, c) == kMstArgsSamples);
    EXPECT(mst_check_args(x, 8, 4, 4, 9, a, b, w, c) == kMstArgsSamples);  // > n
    EXPECT(mst_check_args(x, 1000, 1, 1, kKnnKMax, a, b, w, c) == kMstArgsOk);
    EXPECT(mst_check_args(x, 1000, 1, 1, kKnnKMax + 1, a, b, w, c) == kMstArgsSamples);
    // null pointers
    EXPECT(mst_check_args(nullptr, 8, 4, 4, 1, a, b, w, c) == kMstArgsNull);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, nullptr, b, w, c) == kMstArgsNull);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a, nullptr, w, c) == kMstArgsNull);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a, b, nullptr, c) == kMstArgsNull);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a, b, w, nullptr) == kMstArgsNull);
    EXPECT(mst_check_args(x, 1, 4, 4, 1, nullptr, nullptr, nullptr, nullptr) == kMstArgsNull);
    // alignment
    const char* xc = reinterpret_cast<const char*>(x);
    EXPECT(mst_check_args(xc + 4, 7, 4, 4, 1, a, b, w, c) == kMstArgsAlign);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a, b, reinterpret_cast<char*>(w) + 4, c) == kMstArgsAlign);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a, b, w, reinterpret_cast<char*>(c) + 4) == kMstArgsAlign);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, reinterpret_cast<char*>(a) + 2, b, w, c) == kMstArgsAlign);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a, reinterpret_cast<char*>(b) + 2, w, c) == kMstArgsAlign);
    EXPECT(mst_check_args(x, 8, 4, 4, 1, a + 1, b + 1, w, c) == kMstArgsOk);  // a and b owe 4 bytes only
    // byte sizes: n * ld * 8 in 63 bits
    const int64_t big = int64_t(1) << 40;
    EXPECT(mst_check_args(x, int64_t(1) << 20, 4, big, 1, a, b, w, c) == kMstArgsBytes);      // 2^63
    EXPECT(mst_check_args(x, (int64_t(1) << 20) - 1, 4, big, 1, a, b, w, c) == kMstArgsOk);   // just below
    EXPECT(mst_check_args(x, 3, 4, INT64_MAX, 1, a, b, w, c) == kMstArgsBytes);
    // the first failing check names the error: order of the checks
    EXPECT(mst_check_args(nullptr, 8, 4, 3, 0, nullptr, nullptr, nullptr, nullptr) == kMstArgsStride);
    EXPECT(mst_check_args(nullptr, 8, 4, 4, 0, nullptr, nullptr, nullptr, nullptr) == kMstArgsSamples);
    for (int e = kMstArgsShape; e <= kMstArgsBytes; ++e) EXPECT(mst_arg_message((MstArgError)e)[0] != 0);
    EXPECT(mst_arg_message(kMstArgsOk)[0] == 0);

    // rounds: ceil(log2 n)
    EXPECT(mst_rounds_max(1) == 0 && mst_rounds_max(2) == 1 && mst_rounds_max(3) == 2 && mst_rounds_max(4) == 2);
    EXPECT(mst_rounds_max(5) == 3 && mst_rounds_max(1024) == 10 && mst_rounds_max(1025) == 11);
    EXPECT(mst_rounds_max(200000) == 18 && mst_rounds_max(kKnnMaxRows - 1) == 31);
    // the split: within the capacity, the tiles and the limit; at least 1
    EXPECT(mst_split(1, 512) == 1 && mst_split(kKnnC, 512) == 1 && mst_split(kKnnC + 1, 512) == 2);
    EXPECT(mst_split(10 * kKnnC, 512) == 10 && mst_split(100 * kKnnC, 512) == 5 && mst_split(100 * kKnnC, 0) == 1);
    EXPECT(mst_split(40 * kKnnC, 1 << 20) == kMstSplitMax && mst_split(200000, 512) == 1);
    for (int64_t n : {int64_t(1), int64_t(127), int64_t(129), int64_t(5000), int64_t(200000), kKnnMaxRows - 1})
        for (int64_t cap : {int64_t(0), int64_t(1), int64_t(512), int64_t(1) << 40}) {
            const int s = mst_split(n, cap);
            EXPECT(s >= 1 && s <= kMstSplitMax && s <= (n + kKnnC - 1) / kKnnC);
        }

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
