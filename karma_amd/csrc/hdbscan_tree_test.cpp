// hdbscan_tree_test.cpp — karma_hdbscan_tree (hdbscan_tree.cpp) on the host,
// built with AddressSanitizer + UBSan (make hdbscan_tree_test;
// tests/test_hdbscan_tree_cpu.py): the argument and edge checks, hand-worked
// small trees, and random trees whose results must be well formed.  The
// comparison with the numpy model is the Python test's.  No GPU code.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/karma.h"
#include "hdbscan_tree.h"

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

struct Result {
    int rc;
    std::vector<int32_t> labels;
    std::vector<double> prob;
    int32_t clusters;
};

static Result run(int64_t n, const std::vector<int32_t>& a, const std::vector<int32_t>& b, const std::vector<double>& w,
                  int min_size, int single) {
    Result r{0, std::vector<int32_t>((size_t)std::max<int64_t>(n, 1), -7),
             std::vector<double>((size_t)std::max<int64_t>(n, 1), -7.0), -7};
    r.rc = karma_hdbscan_tree(n, a.data(), b.data(), w.data(), min_size, single, r.labels.data(), r.prob.data(),
                              &r.clusters);
    return r;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random() {
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return g_state;
}

int main() {
    // one point, two points
    Result r = run(1, {}, {}, {}, 2, 0);
    EXPECT(r.rc == KARMA_OK && r.labels[0] == -1 && r.prob[0] == 0.0 && r.clusters == 0);
    r = run(1, {}, {}, {}, 5, 1);
    EXPECT(r.rc == KARMA_OK && r.labels[0] == -1 && r.prob[0] == 0.0 && r.clusters == 0);
    r = run(2, {0}, {1}, {2.0}, 2, 0);
    EXPECT(r.rc == KARMA_OK && r.clusters == 0 && r.labels[0] == -1 && r.labels[1] == -1 && r.prob[0] == 0.0);
    r = run(2, {0}, {1}, {2.0}, 2, 1);
    EXPECT(r.rc == KARMA_OK && r.clusters == 1 && r.labels[0] == 0 && r.labels[1] == 0);
    EXPECT(r.prob[0] == 1.0 && r.prob[1] == 1.0);

    // two tight pairs far apart, and a straggler: {0, 1} and {2, 3} are clusters, 4 leaves the root first
    {
        const std::vector<int32_t> a{0, 2, 1, 3}, b{1, 3, 2, 4};
        const std::vector<double> w{1.0, 2.0, 8.0, 16.0};
        r = run(5, a, b, w, 2, 0);
        EXPECT(r.rc == KARMA_OK && r.clusters == 2);
        EXPECT(r.labels[0] == 0 && r.labels[1] == 0 && r.labels[2] == 1 && r.labels[3] == 1 && r.labels[4] == -1);
        EXPECT(r.prob[0] == 1.0 && r.prob[1] == 1.0 && r.prob[2] == 1.0 && r.prob[3] == 1.0 && r.prob[4] == 0.0);
    }

    // errors: nothing is written
    r = run(0, {}, {}, {}, 2, 0);
    EXPECT(r.rc == KARMA_ERR_ARG && r.clusters == -7);
    r = run(3, {0, 1}, {1, 2}, {1.0, 2.0}, 1, 0);  // min_cluster_size < 2
    EXPECT(r.rc == KARMA_ERR_ARG && r.labels[0] == -7);
    r = run(3, {0, 1}, {1, 2}, {2.0, 1.0}, 2, 0);  // unsorted
    EXPECT(r.rc == KARMA_ERR_ARG && r.labels[0] == -7 && r.prob[2] == -7.0 && r.clusters == -7);
    r = run(3, {0, 1}, {1, 2}, {1.0, std::nan("")}, 2, 0);
    EXPECT(r.rc == KARMA_ERR_ARG);
    r = run(3, {0, 1}, {1, 2}, {-1.0, 2.0}, 2, 0);
    EXPECT(r.rc == KARMA_ERR_ARG);
    r = run(3, {0, 1}, {1, 3}, {1.0, 2.0}, 2, 0);  // endpoint out of range
    EXPECT(r.rc == KARMA_ERR_ARG && r.labels[0] == -7);
    r = run(3, {0, -1}, {1, 2}, {1.0, 2.0}, 2, 0);
    EXPECT(r.rc == KARMA_ERR_ARG);
    r = run(3, {0, 1}, {1, 0}, {1.0, 2.0}, 2, 0);  // a cycle
    EXPECT(r.rc == KARMA_ERR_ARG && r.labels[0] == -7);
    r = run(3, {0, 1}, {1, 1}, {1.0, 2.0}, 2, 0);  // a loop
    EXPECT(r.rc == KARMA_ERR_ARG);
    {
        int32_t lab[3], cnt = 0;
        double pr[3];
        const int32_t a[2] = {0, 1}, b[2] = {1, 2};
        const double w[2] = {1.0, 2.0};
        EXPECT(karma_hdbscan_tree(3, nullptr, b, w, 2, 0, lab, pr, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_hdbscan_tree(3, a, b, w, 2, 0, nullptr, pr, &cnt) == KARMA_ERR_ARG);
        EXPECT(karma_hdbscan_tree(3, a, b, w, 2, 0, lab, pr, nullptr) == KARMA_ERR_ARG);
        EXPECT(karma_hdbscan_tree(3, a, b, w, 2, 0, lab, pr, &cnt) == KARMA_OK);
    }

    // random trees (random attachment, chains and stars among them), ties and zero weights included: the
    // result is well formed
    for (int trial = 0; trial < 300; ++trial) {
        const int64_t n = 1 + (int64_t)(next_random() % 400);
        const int shape = trial % 4;
        std::vector<int32_t> a, b;
        std::vector<double> w;
        for (int64_t i = 1; i < n; ++i) {
            const int64_t to = shape == 0 ? (int64_t)(next_random() % (uint64_t)i) : shape == 1 ? i - 1 : shape == 2 ? 0
                                          : std::max<int64_t>(0, i - 1 - (int64_t)(next_random() % 3));
            a.push_back((int32_t)std::min(i, to)), b.push_back((int32_t)std::max(i, to));
            w.push_back((double)(next_random() % (trial % 3 == 0 ? 4 : 1000) + (trial % 5 == 0 ? 0 : 1)) / 8.0);
        }
        std::sort(w.begin(), w.end());
        const int min_size = 2 + (int)(next_random() % 9);
        for (int single = 0; single < 2; ++single) {
            r = run(n, a, b, w, min_size, single);
            EXPECT(r.rc == KARMA_OK && r.clusters >= 0 && r.clusters <= n);
            std::vector<int64_t> members((size_t)r.clusters + 1, 0);
            bool ok = true;
            for (int64_t i = 0; i < n; ++i) {
                ok = ok && r.labels[i] >= -1 && r.labels[i] < r.clusters;
                if (!ok) break;
                ++members[(size_t)(r.labels[i] + 1)];
                // (a probability is NaN only beside a zero weight: outside the contract)
                ok = ok && (r.labels[i] >= 0 || r.prob[i] == 0.0) && !(r.prob[i] < 0.0) && !(r.prob[i] > 1.0);
            }
            EXPECT(ok);
            for (int32_t c = 0; c < r.clusters; ++c) EXPECT(members[(size_t)c + 1] >= (single ? 1 : min_size));
        }
    }

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
