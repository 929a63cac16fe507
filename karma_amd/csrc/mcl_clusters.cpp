// mcl_clusters.cpp — karma_mcl_clusters: the clusters of a final MCL matrix, on
// the host (no device, no context; include/karma.h has the contract).
// Attractors are the nodes with a diagonal entry; attractor systems their
// connected components; every node joins the system that holds the largest
// in-order mass of its column.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/karma.h"
#include "mcl_args.h"

namespace karma {
void set_error(const char* fmt, ...);  // core.hip, or the stand-alone test program's own
}

namespace {

int64_t find_root(std::vector<int64_t>& parent, int64_t x) {
    while (parent[(size_t)x] != x) {
        parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
        x = parent[(size_t)x];
    }
    return x;
}

int clusters(int64_t n, const int64_t* colptr, const uint32_t* rows, const double* vals, int32_t* labels,
             int32_t* n_clusters) {
    const size_t N = (size_t)n;
    std::vector<uint8_t> attractor(N, 0);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t t = colptr[j]; t < colptr[j + 1]; ++t)
            if ((int64_t)rows[t] == j) attractor[(size_t)j] = 1;
    // attractor systems: a ~ b when T[a, b] is present (that covers T[b, a], seen from column a)
    std::vector<int64_t> parent(N);
    std::iota(parent.begin(), parent.end(), int64_t(0));
    for (int64_t b = 0; b < n; ++b) {
        if (!attractor[(size_t)b]) continue;
        for (int64_t t = colptr[b]; t < colptr[b + 1]; ++t) {
            const int64_t a = rows[t];
            if (!attractor[(size_t)a]) continue;
            const int64_t ra = find_root(parent, a), rb = find_root(parent, b);
            if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);  // the root is the smallest attractor
        }
    }
    // a node's cluster: its system's smallest attractor, or n + j for a node of its own
    std::vector<int64_t> cluster(N);
    std::vector<double> mass(N, 0.0);
    std::vector<int64_t> touched;
    for (int64_t j = 0; j < n; ++j) {
        touched.clear();
        for (int64_t t = colptr[j]; t < colptr[j + 1]; ++t) {
            const int64_t a = rows[t];
            if (!attractor[(size_t)a]) continue;
            const int64_t r = find_root(parent, a);
            if (std::find(touched.begin(), touched.end(), r) == touched.end()) {
                touched.push_back(r);
                mass[(size_t)r] = 0.0;
            }
            mass[(size_t)r] = mass[(size_t)r] + vals[t];  // row ascending, from +0.0
        }
        int64_t best = -1;
        for (int64_t r : touched)
            if (best < 0 || mass[(size_t)r] > mass[(size_t)best] || (mass[(size_t)r] == mass[(size_t)best] && r < best))
                best = r;
        cluster[(size_t)j] = best < 0 ? n + j : best;
    }
    // labels: rank under (size descending, smallest member ascending)
    std::vector<int64_t> order(N);
    std::iota(order.begin(), order.end(), int64_t(0));
    std::stable_sort(order.begin(), order.end(),
                     [&](int64_t x, int64_t y) { return cluster[(size_t)x] < cluster[(size_t)y]; });
    struct Group {
        int64_t size, first, id;
    };
    std::vector<Group> groups;
    for (size_t p = 0; p < N; ++p) {
        const int64_t j = order[p];
        if (p == 0 || cluster[(size_t)j] != cluster[(size_t)order[p - 1]])
            groups.push_back({0, j, cluster[(size_t)j]});  // stable: j is the group's smallest member
        ++groups.back().size;
    }
    std::sort(groups.begin(), groups.end(),
              [](const Group& x, const Group& y) { return x.size != y.size ? x.size > y.size : x.first < y.first; });
    // cluster id -> label through the members themselves
    std::vector<int32_t> label_of_first(N, -1);
    for (size_t g = 0; g < groups.size(); ++g) label_of_first[(size_t)groups[g].first] = (int32_t)g;
    int32_t cur = -1;
    for (size_t p = 0; p < N; ++p) {
        const int64_t j = order[p];
        if (p == 0 || cluster[(size_t)j] != cluster[(size_t)order[p - 1]]) cur = label_of_first[(size_t)j];
        labels[(size_t)j] = cur;
    }
    *n_clusters = (int32_t)groups.size();
    return KARMA_OK;
}

}  // namespace

extern "C" int karma_mcl_clusters(int64_t n, const int64_t* colptr, const uint32_t* rows, const double* vals,
                                  int32_t* labels, int32_t* n_clusters) {
    const karma::MclArgError bad = karma::mcl_check_matrix(n, colptr, rows, vals, labels, n_clusters);
    if (bad != karma::kMclArgsOk) {
        karma::set_error("%s", karma::mcl_arg_message(bad));
        return KARMA_ERR_ARG;
    }
    try {
        return clusters(n, colptr, rows, vals, labels, n_clusters);
    } catch (const std::bad_alloc&) {
        karma::set_error("karma_mcl_clusters: out of host memory for %lld nodes", (long long)n);
        return KARMA_ERR_OOM;
    }
}
