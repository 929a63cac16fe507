// umap_math.h — the defined functions of the device UMAP (include/karma.h):
// kexp / klog / kpow, the counter-based generator, one row's smooth-kNN sigma
// and one vertex's epoch of the layout.  Host and device alike: every step is a
// single IEEE f64 + - * /, a comparison, rint, floor, frexp or ldexp, so a file
// compiled without contraction and without fast-math gives the bits the numpy
// model (tests/umap_reference.py) gives.  No HIP header is needed to include it.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KARMA_HD __host__ __device__ inline
#else
#define KARMA_HD inline
#endif
#if defined(__clang__)
#define KARMA_UNROLL _Pragma("unroll")
#else
#define KARMA_UNROLL
#endif

namespace karma {

constexpr double kUmapLog2e = 1.4426950408889634;
constexpr double kUmapLn2Hi = 6.93147180369123816490e-01;
constexpr double kUmapLn2Lo = 1.90821492927058770002e-10;
constexpr uint64_t kUmapGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kUmapEdgeMul = 0xD1342543DE82EF95ull;
constexpr int kUmapMaxDim = 16;
constexpr int kUmapBisections = 64;

KARMA_HD double kexp(double x) {
    x = x < -745.0 ? -745.0 : x;
    x = x > 709.0 ? 709.0 : x;
    const double n = rint(x * kUmapLog2e);
    const double r = (x - n * kUmapLn2Hi) - n * kUmapLn2Lo;
    // 1 / d!: the correctly rounded quotients (the divisions are folded as IEEE divisions)
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double h = floor(n * 0.5);
    return ldexp(ldexp(p, (int)h), (int)(n - h));
}

// x > 0, finite
KARMA_HD double klog(double x) {
    int ei = 0;
    double m = frexp(x, &ei);
    if (m < 0.7071067811865476) {
        m = m * 2.0;
        ei = ei - 1;
    }
    const double e = (double)ei;
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    return e * kUmapLn2Hi + ((2.0 * s) * p + e * kUmapLn2Lo);
}

// x > 0
KARMA_HD double kpow(double x, double b) { return kexp(b * klog(x)); }

// the finaliser of the project's synthetic generator (synth.cpp)
KARMA_HD uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the uniform [-10, 10) start of coordinate `flat` = i * dim + c
KARMA_HD double umap_init_value(uint64_t seed, uint64_t flat) {
    const uint64_t u = splitmix64(seed + (flat + 1) * kUmapGolden) >> 11;
    return -10.0 + 20.0 * ((double)u * 0x1p-53);
}

KARMA_HD double umap_clip4(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

// rho and the in-order sum of one row's k distances
KARMA_HD void umap_row_rho(const double* dist, int k, double* rho, double* row_sum) {
    double s = 0.0, first = 0.0;
    for (int j = 0; j < k; ++j) {
        const double d = dist[j];
        s = s + d;
        if (first == 0.0 && d > 0.0) first = d;
    }
    *rho = first;
    *row_sum = s;
}

// smooth_knn_dist's bisection for row i, with the floor
KARMA_HD double umap_row_sigma(const int32_t* idx, const double* dist, int k, int64_t i, double rho, double row_sum,
                               double global_mean, double target) {
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < kUmapBisections; ++it) {
        double psum = 0.0;
        for (int j = 0; j < k; ++j) {
            if ((int64_t)idx[j] == i) continue;
            const double d = dist[j] - rho;
            psum = psum + (d > 0.0 ? kexp(-(d / mid)) : 1.0);
        }
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double mean = rho > 0.0 ? row_sum / (double)k : global_mean;
    const double floor_v = 1e-3 * mean;
    return mid > floor_v ? mid : floor_v;
}

// the membership of a non-self entry
KARMA_HD double umap_membership(double dist, double rho, double sigma) {
    const double d = dist - rho;
    return (d <= 0.0 || sigma == 0.0) ? 1.0 : kexp(-(d / sigma));
}

// One move of `cur` against the point `o`; attract: g from the attraction, else the repulsion.
template <int DIM, bool ATTRACT>
KARMA_HD void umap_move(double (&cur)[DIM], const double* o, double a, double b, double gamma, double alpha) {
    double df[DIM];
    double d2 = 0.0;
    KARMA_UNROLL
    for (int c = 0; c < DIM; ++c) {
        df[c] = cur[c] - o[c];
        d2 = d2 + df[c] * df[c];
    }
    if (!(d2 > 0.0)) return;
    const double pb = kpow(d2, b);
    const double g = ATTRACT ? ((-2.0 * a * b) * (pb / d2)) / (a * pb + 1.0)
                             : (2.0 * gamma * b) / ((0.001 + d2) * (a * pb + 1.0));
    KARMA_UNROLL
    for (int c = 0; c < DIM; ++c) cur[c] = cur[c] + umap_clip4(g * df[c]) * alpha;
}

// Vertex i's epoch `ep`: walks its row in CSR order, reads every other vertex
// from y_old, keeps its own coordinates live, writes y_new[i].  eps, eons,
// eonns and t are the per-entry schedule (an inactive entry has eons = +inf).
template <int DIM>
KARMA_HD void umap_vertex_epoch(int64_t i, int64_t n, const int64_t* indptr, const int32_t* indices,
                                const double* eps, double* eons, double* eonns, uint32_t* t, const double* y_old,
                                double* y_new, int ep, double alpha, double a, double b, double gamma, int R,
                                uint64_t seed) {
    double cur[DIM];
    KARMA_UNROLL
    for (int c = 0; c < DIM; ++c) cur[c] = y_old[i * DIM + c];
    const double fep = (double)ep;
    const int64_t e_hi = indptr[i + 1];
    for (int64_t e = indptr[i]; e < e_hi; ++e) {
        const double eo = eons[e];
        if (!(eo <= fep)) continue;
        const double ee = eps[e];
        umap_move<DIM, true>(cur, y_old + (int64_t)indices[e] * DIM, a, b, gamma, alpha);
        eons[e] = eo + ee;
        if (R > 0) {
            const double epns = ee / (double)R;
            const double en = eonns[e];
            const int nneg = (int)((fep - en) / epns);
            const uint64_t base = seed ^ ((uint64_t)e * kUmapEdgeMul);
            uint32_t te = t[e];
            for (int p = 0; p < nneg; ++p) {
                const uint64_t kk = splitmix64(base + ((uint64_t)te + 1) * kUmapGolden) % (uint64_t)n;
                te += 1;
                umap_move<DIM, false>(cur, y_old + (int64_t)kk * DIM, a, b, gamma, alpha);
            }
            t[e] = te;
            eonns[e] = en + (double)nneg * epns;
        }
    }
    KARMA_UNROLL
    for (int c = 0; c < DIM; ++c) y_new[i * DIM + c] = cur[c];
}

}  // namespace karma
