// hdbscan_tree.h — HDBSCAN's host tail: from the edges of a minimum spanning
// tree to labels and membership probabilities (karma_hdbscan_tree).  A pure
// host header (no HIP), shared by hdbscan_tree.cpp and hdbscan_tree_test.cpp.
//
// The steps (include/karma.h has the contract):
//   1. single linkage: a union-find walks the n - 1 edges in the order given
//      (non-decreasing weight); merge e makes node n + e of left = find(a),
//      right = find(b);
//   2. condensing, breadth-first from the root (left before right), with
//      lambda = 1 / w (+inf for w == 0): a split with both sides of at least
//      min_cluster_size points makes two new clusters, the left one numbered
//      first; otherwise the large side keeps its parent's label and the points
//      of a small side fall out of that label at that lambda (listed
//      breadth-first);
//   3. stability of a label: the sum, in the order the condensed entries were
//      made, of (lambda - lambda at which the label was born) * size;
//   4. excess of mass, from the deepest label up; the root only with
//      allow_single_cluster;
//   5. labels 0.. by ascending selected label, noise -1; probabilities.
#pragma once

#include <cstdint>

namespace karma {

enum HdbscanTreeError : int {
    kTreeOk = 0,
    kTreeShape,     // n < 1 or n >= 2^31, or min_cluster_size < 2
    kTreeNull,      // a null pointer that would be read or written
    kTreeWeight,    // a weight that is negative or NaN, or smaller than the one before it
    kTreeEndpoint,  // an endpoint outside [0, n)
    kTreeCycle,     // an edge whose endpoints are joined already
};

inline const char* hdbscan_tree_message(HdbscanTreeError e) {
    switch (e) {
        case kTreeShape: return "need 1 <= n < 2^31 and min_cluster_size >= 2";
        case kTreeNull: return "null pointer";
        case kTreeWeight: return "weights must be >= 0 and must not decrease";
        case kTreeEndpoint: return "an edge's endpoint is not in [0, n)";
        case kTreeCycle: return "an edge joins two points that earlier edges have joined (not a tree)";
        default: return "";
    }
}

// Checks the arguments and the edges, then writes labels[n], prob[n] and
// *n_clusters.  Nothing is written on an error.  Throws std::bad_alloc.
HdbscanTreeError hdbscan_tree_labels(int64_t n, const int32_t* a, const int32_t* b, const double* w,
                                     int min_cluster_size, bool allow_single_cluster, int32_t* labels, double* prob,
                                     int32_t* n_clusters);

}  // namespace karma
