// hdbscan_tree.cpp — karma_hdbscan_tree: single linkage, condensed tree, excess
// of mass and labels on the host (hdbscan_tree.h).  No HIP header: built like
// ingest.cpp, and with sanitizers in hdbscan_tree_test.
#include "hdbscan_tree.h"

#include <cmath>
#include <limits>
#include <new>
#include <vector>

#include "../../include/karma.h"

namespace karma {
void set_error(const char* fmt, ...);

namespace {

int64_t find_root(std::vector<int64_t>& up, int64_t x) {
    int64_t r = x;
    while (up[r] != r) r = up[r];
    while (up[x] != r) {
        const int64_t next = up[x];
        up[x] = r;
        x = next;
    }
    return r;
}

// nodes 0 .. n - 1 are points; node n + e is merge e
struct Linkage {
    int64_t n = 0;
    std::vector<int64_t> left, right, size;  // per merge
    std::vector<double> w;
    int64_t count(int64_t node) const { return node < n ? 1 : size[node - n]; }
};

// the nodes below (and with) `from`, breadth-first, left before right
void breadth_first(const Linkage& t, int64_t from, std::vector<int64_t>& out) {
    out.clear();
    out.push_back(from);
    for (size_t head = 0; head < out.size(); ++head) {
        const int64_t node = out[head];
        if (node < t.n) continue;
        out.push_back(t.left[node - t.n]);
        out.push_back(t.right[node - t.n]);
    }
}

// The condensed tree, one entry per (parent label, child): a child below n is a
// point that falls out of the label, any other a new cluster label.  Labels
// count from n (the root) in the order they are made.
struct CondensedTree {
    std::vector<int64_t> parent, child, size;
    std::vector<double> lambda;
    int64_t labels = 0;  // cluster labels made: n ... n + labels - 1
};

CondensedTree condense(const Linkage& t, int64_t min_size) {
    CondensedTree c;
    const int64_t n = t.n, root = 2 * n - 2;
    std::vector<int64_t> order, sub;
    breadth_first(t, root, order);
    std::vector<int64_t> relabel(root + 1, -1);
    std::vector<char> gone(root + 1, 0);
    relabel[root] = n;
    int64_t next_label = n + 1;
    auto entry = [&](int64_t p, int64_t ch, double lam, int64_t sz) {
        c.parent.push_back(p), c.child.push_back(ch), c.lambda.push_back(lam), c.size.push_back(sz);
    };
    auto fall_out = [&](int64_t from, int64_t label, double lam) {
        breadth_first(t, from, sub);
        for (int64_t s : sub) {
            if (s < n) entry(label, s, lam, 1);
            gone[s] = 1;
        }
    };
    for (int64_t node : order) {
        if (node < n || gone[node]) continue;
        const int64_t l = t.left[node - n], r = t.right[node - n];
        const double dist = t.w[node - n];
        const double lam = dist > 0.0 ? 1.0 / dist : std::numeric_limits<double>::infinity();
        const int64_t lc = t.count(l), rc = t.count(r);
        const int64_t label = relabel[node];
        if (lc >= min_size && rc >= min_size) {
            relabel[l] = next_label++;
            entry(label, relabel[l], lam, lc);
            relabel[r] = next_label++;
            entry(label, relabel[r], lam, rc);
        } else if (lc < min_size && rc < min_size) {
            fall_out(l, label, lam);
            fall_out(r, label, lam);
        } else if (lc < min_size) {
            relabel[r] = label;
            fall_out(l, label, lam);
        } else {
            relabel[l] = label;
            fall_out(r, label, lam);
        }
    }
    c.labels = next_label - n;
    return c;
}

}  // namespace

HdbscanTreeError hdbscan_tree_labels(int64_t n, const int32_t* a, const int32_t* b, const double* w,
                                     int min_cluster_size, bool allow_single_cluster, int32_t* labels, double* prob,
                                     int32_t* n_clusters) {
    if (n < 1 || n >= (int64_t(1) << 31) || min_cluster_size < 2) return kTreeShape;
    if (!labels || !prob || !n_clusters || (n > 1 && (!a || !b || !w))) return kTreeNull;

    // 1. single linkage (and the checks of the edges)
    Linkage t;
    t.n = n;
    const int64_t E = n - 1;
    t.left.resize(E), t.right.resize(E), t.size.resize(E), t.w.resize(E);
    {
        std::vector<int64_t> up(2 * n - 1);
        for (int64_t i = 0; i < 2 * n - 1; ++i) up[i] = i;
        for (int64_t e = 0; e < E; ++e) {
            if (!(w[e] >= 0.0) || (e > 0 && w[e] < w[e - 1])) return kTreeWeight;
            if (a[e] < 0 || a[e] >= n || b[e] < 0 || b[e] >= n) return kTreeEndpoint;
            const int64_t l = find_root(up, a[e]), r = find_root(up, b[e]);
            if (l == r) return kTreeCycle;
            t.left[e] = l, t.right[e] = r, t.w[e] = w[e];
            t.size[e] = t.count(l) + t.count(r);
            up[l] = up[r] = n + e;
        }
    }
    if (n == 1) {
        labels[0] = -1, prob[0] = 0.0, *n_clusters = 0;
        return kTreeOk;
    }

    // 2. the condensed tree
    const CondensedTree c = condense(t, min_cluster_size);
    const int64_t K = c.labels, entries = (int64_t)c.parent.size();

    // 3. stability; a cluster's parent label, its (at most two) child labels, its largest lambda
    std::vector<double> birth(K, 0.0), stability(K, 0.0), max_lambda(K, 0.0);
    std::vector<int64_t> up(K, -1), kid0(K, -1), kid1(K, -1);
    for (int64_t i = 0; i < entries; ++i) {
        const int64_t p = c.parent[i] - n;
        if (c.child[i] >= n) {
            const int64_t ch = c.child[i] - n;
            birth[ch] = c.lambda[i];
            up[ch] = p;
            (kid0[p] < 0 ? kid0[p] : kid1[p]) = ch;
        }
    }
    std::vector<char> seen(K, 0);
    for (int64_t i = 0; i < entries; ++i) {
        const int64_t p = c.parent[i] - n;
        stability[p] += (c.lambda[i] - birth[p]) * (double)c.size[i];
        if (!seen[p] || c.lambda[i] > max_lambda[p]) max_lambda[p] = c.lambda[i], seen[p] = 1;
    }

    // 4. excess of mass, deepest label first (a child's label is above its parent's)
    std::vector<char> selected(K, 1);
    if (!allow_single_cluster) selected[0] = 0;
    std::vector<int64_t> stack;
    for (int64_t k = K - 1; k >= (allow_single_cluster ? 0 : 1); --k) {
        double below = 0.0;
        if (kid0[k] >= 0) below = stability[kid0[k]] + stability[kid1[k]];
        if (below > stability[k]) {
            selected[k] = 0;
            stability[k] = below;
        } else {
            stack.clear();
            if (kid0[k] >= 0) stack.push_back(kid0[k]), stack.push_back(kid1[k]);
            while (!stack.empty()) {
                const int64_t s = stack.back();
                stack.pop_back();
                selected[s] = 0;
                if (kid0[s] >= 0) stack.push_back(kid0[s]), stack.push_back(kid1[s]);
            }
        }
    }

    // 5. numbers of the selected labels, ascending; the selected label a label's points belong to
    std::vector<int64_t> number(K, -1), home(K, -1);
    int64_t count = 0;
    for (int64_t k = 0; k < K; ++k)
        if (selected[k]) number[k] = count++;
    for (int64_t k = 0; k < K; ++k) home[k] = selected[k] ? k : (k == 0 ? -1 : home[up[k]]);
    const bool lone_root = allow_single_cluster && count == 1 && selected[0];

    for (int64_t i = 0; i < n; ++i) labels[i] = -1, prob[i] = 0.0;
    for (int64_t i = 0; i < entries; ++i) {
        const int64_t pt = c.child[i];
        if (pt >= n) continue;
        const int64_t h = home[c.parent[i] - n];
        if (h < 0) continue;
        // the root alone: a point belongs to it when it stays at least as long as any of the root's children
        if (h == 0 && !(lone_root && c.lambda[i] >= max_lambda[0])) continue;
        labels[pt] = (int32_t)number[h];
        const double top = max_lambda[h];
        if (top == 0.0 || !std::isfinite(top)) prob[pt] = 1.0;
        else prob[pt] = (c.lambda[i] < top ? c.lambda[i] : top) / top;
    }
    *n_clusters = (int32_t)count;
    return kTreeOk;
}

}  // namespace karma

extern "C" int karma_hdbscan_tree(int64_t n, const int32_t* a, const int32_t* b, const double* w, int min_cluster_size,
                                  int allow_single_cluster, int32_t* labels, double* prob, int32_t* n_clusters) {
    try {
        const karma::HdbscanTreeError bad = karma::hdbscan_tree_labels(n, a, b, w, min_cluster_size,
                                                                       allow_single_cluster != 0, labels, prob, n_clusters);
        if (bad != karma::kTreeOk) {
            karma::set_error("karma_hdbscan_tree: %s", karma::hdbscan_tree_message(bad));
            return KARMA_ERR_ARG;
        }
    } catch (const std::bad_alloc&) {
        karma::set_error("karma_hdbscan_tree: out of host memory");
        return KARMA_ERR_OOM;
    }
    return KARMA_OK;
}
