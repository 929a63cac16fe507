// knn_args_test.cpp — karma_knn_rows' argument checks (knn_args.h) on the host,
// built with AddressSanitizer + UBSan (make knn_args_test;
// tests/test_knn_args_cpu.py).  No GPU code.
#include <cstdio>
#include <vector>

#include "knn_args.h"

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
    static_assert(kKnnKMax >= 64, "UMAP's default is 15; the contract promises at least 64");
    static_assert(kKnnKMax == 64, "knn_arg_message names the limit");
    static_assert(kKnnQ % 32 == 0 && kKnnC % 32 == 0 && kKnnThreads == 256, "8 x 8 pairs per thread of a 16 x 16 grid");
    static_assert(kKnnQ * kKnnC == kKnnThreads * 64, "every pair of two tiles has a thread");

    std::vector<double> xs(64), ds(64);
    std::vector<int32_t> is(64);
    const double* x = xs.data();
    double* d = ds.data();
    int32_t* i = is.data();

    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 3, i, d) == kKnnArgsOk);
    EXPECT(knn_check_args(x, 8, 4, 7, 2, 5, 8, i, d) == kKnnArgsOk);    // ld > m, k == n
    EXPECT(knn_check_args(x, 8, 0, 0, 0, 8, 1, i, d) == kKnnArgsOk);    // no columns: every d2 is +0
    EXPECT(knn_check_args(nullptr, 8, 0, 0, 0, 8, 1, i, d) == kKnnArgsOk);
    // nothing to do: neither pointers nor k are looked at
    EXPECT(knn_check_args(nullptr, 0, 4, 4, 0, 0, 0, nullptr, nullptr) == kKnnArgsOk);
    EXPECT(knn_check_args(nullptr, 8, 4, 4, 3, 3, -5, nullptr, nullptr) == kKnnArgsOk);
    EXPECT(knn_check_args(nullptr, 8, 4, 4, 8, 8, 99, nullptr, nullptr) == kKnnArgsOk);
    // shape
    EXPECT(knn_check_args(x, -1, 4, 4, 0, 0, 1, i, d) == kKnnArgsShape);
    EXPECT(knn_check_args(x, 8, -1, 4, 0, 8, 1, i, d) == kKnnArgsShape);
    EXPECT(knn_check_args(x, kKnnMaxRows, 4, 4, 0, 1, 1, i, d) == kKnnArgsShape);
    EXPECT(knn_check_args(x, kKnnMaxRows - 1, 1, 1, 0, 1, 1, i, d) == kKnnArgsOk);
    // stride
    EXPECT(knn_check_args(x, 8, 4, 3, 0, 8, 1, i, d) == kKnnArgsStride);
    EXPECT(knn_check_args(x, 8, 4, -4, 0, 8, 1, i, d) == kKnnArgsStride);
    // row range
    EXPECT(knn_check_args(x, 8, 4, 4, -1, 8, 1, i, d) == kKnnArgsRange);
    EXPECT(knn_check_args(x, 8, 4, 4, 5, 4, 1, i, d) == kKnnArgsRange);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 9, 1, i, d) == kKnnArgsRange);
    EXPECT(knn_check_args(x, 0, 4, 4, 0, 1, 1, i, d) == kKnnArgsRange);
    // k
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 0, i, d) == kKnnArgsK);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, -1, i, d) == kKnnArgsK);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 9, i, d) == kKnnArgsK);     // k > n
    EXPECT(knn_check_args(x, 1000, 1, 1, 0, 8, kKnnKMax, i, d) == kKnnArgsOk);
    EXPECT(knn_check_args(x, 1000, 1, 1, 0, 8, kKnnKMax + 1, i, d) == kKnnArgsK);
    // null pointers
    EXPECT(knn_check_args(nullptr, 8, 4, 4, 0, 8, 1, i, d) == kKnnArgsNull);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 1, nullptr, d) == kKnnArgsNull);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 1, i, nullptr) == kKnnArgsNull);
    // alignment
    const char* c = reinterpret_cast<const char*>(x);
    EXPECT(knn_check_args(c + 4, 7, 4, 4, 0, 7, 1, i, d) == kKnnArgsAlign);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 1, i, reinterpret_cast<const char*>(d) + 4) == kKnnArgsAlign);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 1, reinterpret_cast<const char*>(i) + 2, d) == kKnnArgsAlign);
    EXPECT(knn_check_args(x, 8, 4, 4, 0, 8, 1, i + 1, d) == kKnnArgsOk);  // idx owes 4 bytes only
    // byte sizes: n * ld * 8 and rows * k * 8 in 63 bits
    const int64_t big = int64_t(1) << 40;
    EXPECT(knn_check_args(x, int64_t(1) << 30, 4, big, 0, 1, 1, i, d) == kKnnArgsBytes);        // 2^73
    EXPECT(knn_check_args(x, int64_t(1) << 20, 4, big, 0, 1, 1, i, d) == kKnnArgsBytes);        // 2^63
    EXPECT(knn_check_args(x, (int64_t(1) << 20) - 1, 4, big, 0, 1, 1, i, d) == kKnnArgsOk);     // just below
    EXPECT(knn_check_args(x, 3, 4, INT64_MAX, 0, 1, 1, i, d) == kKnnArgsBytes);
    int64_t b = -1;
    EXPECT(knn_bytes(0, INT64_MAX, INT64_MAX, &b) && b == 0);
    EXPECT(knn_bytes(INT64_MAX, 1, 1, &b) && b == INT64_MAX);
    EXPECT(!knn_bytes(INT64_MAX, 2, 1, &b));
    EXPECT(!knn_bytes(INT64_MAX / 8 + 1, 1, 8, &b));
    EXPECT(knn_bytes(INT64_MAX / 8, 1, 8, &b) && b == (INT64_MAX / 8) * 8);
    // the first failing check names the error: order of the checks
    EXPECT(knn_check_args(nullptr, 8, 4, 3, 9, 2, 0, nullptr, nullptr) == kKnnArgsStride);
    EXPECT(knn_check_args(nullptr, 8, 4, 4, 9, 2, 0, nullptr, nullptr) == kKnnArgsRange);
    EXPECT(knn_check_args(nullptr, 8, 4, 4, 0, 8, 0, nullptr, nullptr) == kKnnArgsK);
    for (int e = kKnnArgsShape; e <= kKnnArgsBytes; ++e) EXPECT(knn_arg_message((KnnArgError)e)[0] != 0);
    EXPECT(knn_arg_message(kKnnArgsOk)[0] == 0);

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
