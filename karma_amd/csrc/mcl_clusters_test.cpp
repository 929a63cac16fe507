// mcl_clusters_test.cpp — karma_mcl_clusters (mcl_clusters.cpp) on the host,
// built with AddressSanitizer + UBSan (make mcl_clusters_test;
// tests/test_mcl_clusters_cpu.py): hand-worked matrices for every rule, the
// argument checks, and, given a file of cases (the Python test writes the
// model's matrices and labels into one), each of them.  No GPU code.
//
// Case file: per case a line "n nnz count", then the n + 1 column offsets, the
// nnz rows, the nnz values as the hexadecimal bits of the f64, the n labels.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/karma.h"

namespace karma {
static char g_error[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace karma

static int g_cases = 0, g_failed = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        ++g_cases;                                                       \
        if (!(cond)) {                                                   \
            ++g_failed;                                                  \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                                \
    } while (0)

struct Column {
    std::vector<uint32_t> rows;
    std::vector<double> vals;
};

struct Result {
    int rc;
    std::vector<int32_t> labels;
    int32_t count;
};

static Result run(const std::vector<Column>& cols) {
    std::vector<int64_t> cp{0};
    std::vector<uint32_t> rows;
    std::vector<double> vals;
    for (const Column& c : cols) {
        rows.insert(rows.end(), c.rows.begin(), c.rows.end());
        vals.insert(vals.end(), c.vals.begin(), c.vals.end());
        cp.push_back((int64_t)rows.size());
    }
    Result r{0, std::vector<int32_t>(cols.size(), -7), -7};
    r.rc = karma_mcl_clusters((int64_t)cols.size(), cp.data(), rows.data(), vals.data(), r.labels.data(), &r.count);
    return r;
}

static int run_file(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) {
        std::printf("cannot open %s\n", path);
        return 1;
    }
    long long n, nnz, count;
    int cases = 0;
    while (std::fscanf(f, "%lld %lld %lld", &n, &nnz, &count) == 3) {
        std::vector<int64_t> cp((size_t)n + 1);
        std::vector<uint32_t> rows((size_t)nnz);
        std::vector<double> vals((size_t)nnz);
        std::vector<int32_t> want((size_t)n), got((size_t)n, -7);
        bool ok = true;
        for (auto& v : cp) ok &= std::fscanf(f, "%" SCNd64, &v) == 1;
        for (auto& v : rows) ok &= std::fscanf(f, "%" SCNu32, &v) == 1;
        for (auto& v : vals) {
            uint64_t bits = 0;
            ok &= std::fscanf(f, "%" SCNx64, &bits) == 1;
            std::memcpy(&v, &bits, 8);
        }
        for (auto& v : want) ok &= std::fscanf(f, "%" SCNd32, &v) == 1;
        EXPECT(ok);
        if (!ok) break;
        int32_t c = -7;
        EXPECT(karma_mcl_clusters(n, cp.data(), rows.data(), vals.data(), got.data(), &c) == KARMA_OK);
        EXPECT(c == (int32_t)count);
        EXPECT(got == want);
        ++cases;
    }
    std::fclose(f);
    std::printf("%d cases from the file\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    // n = 1: an attractor of its own; and a lone node that is none
    Result r = run({{{0}, {1.0}}});
    EXPECT(r.rc == KARMA_OK && r.count == 1 && r.labels[0] == 0);

    // two attractors of one system ({0, 1}, joined through T[0, 1]) and a follower
    r = run({{{0, 1}, {0.5, 0.5}}, {{0, 1}, {0.5, 0.5}}, {{1}, {1.0}}});
    EXPECT(r.rc == KARMA_OK && r.count == 1);
    EXPECT((r.labels == std::vector<int32_t>{0, 0, 0}));

    // a system joined one way only: T[0, 1] present, T[1, 0] absent
    r = run({{{0}, {1.0}}, {{0, 1}, {0.25, 0.75}}});
    EXPECT(r.rc == KARMA_OK && r.count == 1);

    // node 3 split evenly between the systems {0, 1} and {2}: the tie goes to the smallest attractor's system
    r = run({{{0, 1}, {0.5, 0.5}}, {{0, 1}, {0.5, 0.5}}, {{2}, {1.0}}, {{1, 2}, {0.5, 0.5}}});
    EXPECT(r.rc == KARMA_OK && r.count == 2);
    EXPECT((r.labels == std::vector<int32_t>{0, 0, 1, 0}));
    // ... and with the masses 0.25 + 0.25 against 0.5: a system's mass is the sum over its attractors
    r = run({{{0, 1}, {0.5, 0.5}}, {{0, 1}, {0.5, 0.5}}, {{2}, {1.0}}, {{0, 1, 2}, {0.25, 0.25, 0.5}}});
    EXPECT((r.labels == std::vector<int32_t>{0, 0, 1, 0}));
    // the larger mass wins against the smaller attractor
    r = run({{{0}, {1.0}}, {{1}, {1.0}}, {{0, 1}, {0.4, 0.6}}});
    EXPECT(r.rc == KARMA_OK && r.count == 2);
    EXPECT((r.labels == std::vector<int32_t>{1, 0, 0}));  // {1, 2} is the larger cluster

    // nodes without an attractor entry: clusters of their own; entries on non-attractors carry no mass
    r = run({{{0}, {1.0}}, {{2}, {1.0}}, {{1}, {1.0}}, {{0, 1}, {0.1, 0.9}}});
    EXPECT(r.rc == KARMA_OK && r.count == 3);
    EXPECT((r.labels == std::vector<int32_t>{0, 1, 2, 0}));

    // labels: size descending, then smallest member
    r = run({{{0}, {1.0}}, {{1}, {1.0}}, {{1}, {1.0}}, {{4}, {1.0}}, {{4}, {1.0}}, {{4}, {1.0}}});
    EXPECT(r.rc == KARMA_OK && r.count == 3);
    EXPECT((r.labels == std::vector<int32_t>{2, 1, 1, 0, 0, 0}));

    // an attractor may follow another system's larger mass
    r = run({{{0}, {1.0}}, {{0, 1}, {0.9, 0.1}}});
    EXPECT(r.rc == KARMA_OK && r.count == 1);  // 0 ~ 1 through T[0, 1]: one system anyway

    // argument errors: nothing written
    {
        int64_t cp[3] = {0, 1, 2};
        uint32_t rows[2] = {0, 1};
        double vals[2] = {1.0, 1.0};
        int32_t lab[2] = {-7, -7}, cnt = -7;
        EXPECT(karma_mcl_clusters(0, cp, rows, vals, lab, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_mcl_clusters(2, nullptr, rows, vals, lab, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_mcl_clusters(2, cp, nullptr, vals, lab, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_mcl_clusters(2, cp, rows, nullptr, lab, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_mcl_clusters(2, cp, rows, vals, nullptr, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_mcl_clusters(2, cp, rows, vals, lab, nullptr) == KARMA_ERR_ARG);
        rows[1] = 2;
        EXPECT(karma_mcl_clusters(2, cp, rows, vals, lab, &cnt) == KARMA_ERR_ARG);
        rows[1] = 1;
        cp[1] = 0;
        EXPECT(karma_mcl_clusters(2, cp, rows, vals, lab, &cnt) == KARMA_ERR_ARG);
        EXPECT(lab[0] == -7 && lab[1] == -7 && cnt == -7 && karma::g_error[0] != 0);
        cp[1] = 1;
        EXPECT(karma_mcl_clusters(2, cp, rows, vals, lab, &cnt) == KARMA_OK && cnt == 2);
    }

    if (argc > 1 && run_file(argv[1])) return 1;
    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_cases);
        return 1;
    }
    std::printf("ok (%d checks)\n", g_cases);
    return 0;
}
