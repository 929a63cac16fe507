// mcl_args_test.cpp — mcl_args.h on the host, built with AddressSanitizer +
// UBSan (make mcl_args_test; tests/test_mcl_args_cpu.py): every argument check
// of karma_mcl / karma_adj_mcl / karma_mcl_clusters at its limits, the host
// graph check, and the general path's batch arithmetic.  No GPU code.
#include <cstdio>
#include <limits>
#include <vector>

#include "mcl_args.h"

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
    alignas(8) static char buf[256];
    void* p8 = buf;
    void* p4 = buf + 4;
    void* p1 = buf + 1;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // options
    EXPECT(mcl_check_options(2.0, 4, 1.0 / 4000, 1e-3, 100, 0, 0) == kMclArgsOk);
    EXPECT(mcl_check_options(2.0, 2, 0x1p-40, 0.0, 1, 1, kMclMaxSort) == kMclArgsOk);
    EXPECT(mcl_check_options(16.0, 32, 0.5, inf, 1, 0, 1) == kMclArgsOk);
    EXPECT(mcl_check_options(2.0, 1, 0.1, 0.0, 1, 0, 0) == kMclArgsResource);
    EXPECT(mcl_check_options(2.0, 33, 0.1, 0.0, 1, 0, 0) == kMclArgsResource);
    EXPECT(mcl_check_options(1.0, 4, 0.1, 0.0, 1, 0, 0) == kMclArgsInflation);
    EXPECT(mcl_check_options(16.000001, 4, 0.1, 0.0, 1, 0, 0) == kMclArgsInflation);
    EXPECT(mcl_check_options(nan, 4, 0.1, 0.0, 1, 0, 0) == kMclArgsInflation);
    EXPECT(mcl_check_options(2.0, 4, 0x1p-41, 0.0, 1, 0, 0) == kMclArgsCutoff);
    EXPECT(mcl_check_options(2.0, 4, 0.500001, 0.0, 1, 0, 0) == kMclArgsCutoff);
    EXPECT(mcl_check_options(2.0, 4, nan, 0.0, 1, 0, 0) == kMclArgsCutoff);
    EXPECT(mcl_check_options(2.0, 4, 0.1, -1e-300, 1, 0, 0) == kMclArgsEps);
    EXPECT(mcl_check_options(2.0, 4, 0.1, nan, 1, 0, 0) == kMclArgsEps);
    EXPECT(mcl_check_options(2.0, 4, 0.1, 0.0, 0, 0, 0) == kMclArgsIter);
    EXPECT(mcl_check_options(2.0, 4, 0.1, 0.0, 1, 2, 0) == kMclArgsFlags);
    EXPECT(mcl_check_options(2.0, 4, 0.1, 0.0, 1, 0, -1) == kMclArgsCandCap);
    EXPECT(mcl_check_options(2.0, 4, 0.1, 0.0, 1, 0, kMclMaxSort + 1) == kMclArgsCandCap);

    // outputs
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p8, 20, p4, p8) == kMclArgsOk);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p8, 19, p4, p8) == kMclArgsCap);
    EXPECT(mcl_check_outputs(0, 4, p8, p4, p8, 20, p4, p8) == kMclArgsShape);
    EXPECT(mcl_check_outputs(kMclMaxN, 4, p8, p4, p8, INT64_MAX, p4, p8) == kMclArgsShape);
    EXPECT(mcl_check_outputs(kMclMaxN - 1, 32, p8, p4, p8, (kMclMaxN - 1) * 32, p4, p8) == kMclArgsOk);
    EXPECT(mcl_check_outputs(5, 4, nullptr, p4, p8, 20, p4, p8) == kMclArgsNull);
    EXPECT(mcl_check_outputs(5, 4, p8, nullptr, p8, 20, p4, p8) == kMclArgsNull);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, nullptr, 20, p4, p8) == kMclArgsNull);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p8, 20, nullptr, p8) == kMclArgsNull);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p8, 20, p4, nullptr) == kMclArgsNull);
    EXPECT(mcl_check_outputs(5, 4, p4, p4, p8, 20, p4, p8) == kMclArgsAlign);
    EXPECT(mcl_check_outputs(5, 4, p8, p1, p8, 20, p4, p8) == kMclArgsAlign);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p4, 20, p4, p8) == kMclArgsAlign);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p8, 20, p1, p8) == kMclArgsAlign);
    EXPECT(mcl_check_outputs(5, 4, p8, p4, p8, 20, p4, p4) == kMclArgsAlign);

    // the whole call
    EXPECT(mcl_check_args(5, p8, p4, p8, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsOk);
    EXPECT(mcl_check_args(5, p8, nullptr, nullptr, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsOk);
    EXPECT(mcl_check_args(5, nullptr, p4, p8, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsNull);
    EXPECT(mcl_check_args(5, p4, p4, p8, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsAlign);
    EXPECT(mcl_check_args(5, p8, p1, p8, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsAlign);
    EXPECT(mcl_check_args(5, p8, p4, p4, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsAlign);
    EXPECT(mcl_check_args(0, p8, p4, p8, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsShape);
    EXPECT(mcl_check_args(5, p8, p4, p8, 2.0, 40, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 20, p4, p8) == kMclArgsResource);
    EXPECT(mcl_check_args(5, p8, p4, p8, 2.0, 4, 0.1, 0.0, 1, 0, 0, p8, p4, p8, 19, p4, p8) == kMclArgsCap);

    // nnz
    EXPECT(mcl_check_nnz(0, 0, nullptr, nullptr) == kMclArgsOk);
    EXPECT(mcl_check_nnz(0, 3, p4, p8) == kMclArgsOk);
    EXPECT(mcl_check_nnz(0, 3, nullptr, p8) == kMclArgsNull);
    EXPECT(mcl_check_nnz(0, 3, p4, nullptr) == kMclArgsNull);
    EXPECT(mcl_check_nnz(1, 3, p4, p8) == kMclArgsOff);
    EXPECT(mcl_check_nnz(0, -1, p4, p8) == kMclArgsOff);
    EXPECT(mcl_check_nnz(0, kMclMaxN, p4, p8) == kMclArgsOff);
    EXPECT(mcl_check_nnz(0, kMclMaxN - 1, p4, p8) == kMclArgsOk);

    // a host graph's contents
    {
        std::vector<int64_t> seen;
        std::vector<int64_t> off{0, 2, 4, 5, 5};
        std::vector<uint32_t> nbr{1, 2, 0, 1, 0};  // column 1 names itself: ignored
        std::vector<double> w{1.0, 0.5, 1.0, 7.0, 0.5};
        EXPECT(mcl_check_csr(off.data(), nbr.data(), w.data(), 4, seen) == kMclArgsOk);
        auto o2 = off;
        o2[0] = 1;
        EXPECT(mcl_check_csr(o2.data(), nbr.data(), w.data(), 4, seen) == kMclArgsOff);
        o2 = off;
        o2[2] = 1;  // decreasing
        EXPECT(mcl_check_csr(o2.data(), nbr.data(), w.data(), 4, seen) == kMclArgsOff);
        o2 = off;
        o2[3] = 6;  // past off[n]
        EXPECT(mcl_check_csr(o2.data(), nbr.data(), w.data(), 4, seen) == kMclArgsOff);
        auto n2 = nbr;
        n2[4] = 4;
        EXPECT(mcl_check_csr(off.data(), n2.data(), w.data(), 4, seen) == kMclArgsNbr);
        n2 = nbr;
        n2[1] = 1;  // column 0 names 1 twice
        EXPECT(mcl_check_csr(off.data(), n2.data(), w.data(), 4, seen) == kMclArgsDup);
        n2 = nbr;
        n2[2] = 1;  // column 1 names itself twice: both ignored
        EXPECT(mcl_check_csr(off.data(), n2.data(), w.data(), 4, seen) == kMclArgsOk);
        for (double bad : {0.0, -1.0, inf, nan}) {
            auto w2 = w;
            w2[3] = bad;  // a bad weight counts on an ignored entry too
            EXPECT(mcl_check_csr(off.data(), nbr.data(), w2.data(), 4, seen) == kMclArgsWeight);
        }
        std::vector<int64_t> empty{0, 0};
        EXPECT(mcl_check_csr(empty.data(), nullptr, nullptr, 1, seen) == kMclArgsOk);
    }

    // karma_mcl_clusters' matrix
    {
        std::vector<int64_t> cp{0, 2, 3};
        std::vector<uint32_t> rows{0, 1, 1};
        std::vector<double> vals{0.5, 0.5, 1.0};
        int32_t lab[2], cnt;
        EXPECT(mcl_check_matrix(2, cp.data(), rows.data(), vals.data(), lab, &cnt) == kMclArgsOk);
        EXPECT(mcl_check_matrix(0, cp.data(), rows.data(), vals.data(), lab, &cnt) == kMclArgsShape);
        EXPECT(mcl_check_matrix(2, nullptr, rows.data(), vals.data(), lab, &cnt) == kMclArgsNull);
        EXPECT(mcl_check_matrix(2, cp.data(), rows.data(), vals.data(), nullptr, &cnt) == kMclArgsNull);
        EXPECT(mcl_check_matrix(2, cp.data(), rows.data(), vals.data(), lab, nullptr) == kMclArgsNull);
        EXPECT(mcl_check_matrix(2, cp.data(), rows.data(), vals.data(), buf + 1, &cnt) == kMclArgsAlign);
        auto c2 = cp;
        c2[0] = 1;
        EXPECT(mcl_check_matrix(2, c2.data(), rows.data(), vals.data(), lab, &cnt) == kMclArgsColptr);
        c2 = cp;
        c2[1] = 3;  // an empty column
        EXPECT(mcl_check_matrix(2, c2.data(), rows.data(), vals.data(), lab, &cnt) == kMclArgsColptr);
        auto r2 = rows;
        r2[2] = 2;
        EXPECT(mcl_check_matrix(2, cp.data(), r2.data(), vals.data(), lab, &cnt) == kMclArgsNbr);
        r2 = rows;
        r2[0] = 1;  // not ascending
        EXPECT(mcl_check_matrix(2, cp.data(), r2.data(), vals.data(), lab, &cnt) == kMclArgsColptr);
    }

    // batches: whole columns, at most cap candidates, a wide column alone
    {
        const std::vector<int64_t> cc{0, 3, 6, 16, 17, 20};  // counts 3 3 10 1 3
        int64_t eff = 0;
        auto b = mcl_batches(cc.data(), 5, 6, &eff);
        EXPECT(eff == 10);  // raised to the widest column
        EXPECT((b == std::vector<int64_t>{0, 2, 3, 5}));
        b = mcl_batches(cc.data(), 5, 10, &eff);
        EXPECT(eff == 10 && (b == std::vector<int64_t>{0, 2, 3, 5}));
        b = mcl_batches(cc.data(), 5, 11, &eff);
        EXPECT(eff == 11 && (b == std::vector<int64_t>{0, 2, 4, 5}));
        b = mcl_batches(cc.data(), 5, 1, &eff);
        EXPECT(eff == 10 && (b == std::vector<int64_t>{0, 2, 3, 5}));
        b = mcl_batches(cc.data(), 5, 0, &eff);
        EXPECT(eff == kMclCandCap && (b == std::vector<int64_t>{0, 5}));
        b = mcl_batches(cc.data(), 5, 20, &eff);
        EXPECT((b == std::vector<int64_t>{0, 5}));
        b = mcl_batches(cc.data(), 1, 1, &eff);
        EXPECT(eff == 3 && (b == std::vector<int64_t>{0, 1}));
        // every batch within the cap, every column in exactly one batch
        for (int64_t cap = 1; cap <= 21; ++cap) {
            b = mcl_batches(cc.data(), 5, cap, &eff);
            EXPECT(b.front() == 0 && b.back() == 5);
            for (size_t t = 0; t + 1 < b.size(); ++t)
                EXPECT(b[t] < b[t + 1] && cc[(size_t)b[t + 1]] - cc[(size_t)b[t]] <= eff);
        }
    }

    // every error has a message; the constants the kernels are built on
    for (int e = kMclArgsShape; e <= kMclArgsWide; ++e) EXPECT(mcl_arg_message((MclArgError)e)[0] != 0);
    EXPECT(mcl_arg_message(kMclArgsOk)[0] == 0);
    EXPECT(kMclTile * kMclLanesSmall == kMclBlock && kMclBlock % kMclLanesLarge == 0);
    EXPECT(kMclLanesSmall == 4 * 4 && kMclLanesLarge == kMclFusedMaxR * kMclFusedMaxR && kMclLanesLarge == 64);

    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_cases);
        return 1;
    }
    std::printf("ok (%d checks)\n", g_cases);
    return 0;
}
