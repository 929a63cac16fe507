// umap_ab.cpp — karma_umap_ab: umap's find_ab_params on the host.  A least-
// squares fit of 1 / (1 + a x^(2b)) to the membership curve of (spread,
// min_dist) on 300 points of [0, 3 spread], by a small Levenberg-Marquardt
// from a = b = 1.  a and b are inputs of the layout, so its bit contract does
// not rest on this fit (libm's pow / exp / log are fine here).
#include <cmath>

#include "../../include/karma.h"

namespace {

constexpr int kPoints = 300;

struct Fit {
    double x[kPoints], y[kPoints];
};

double cost(const Fit& f, double a, double b) {
    double s = 0.0;
    for (int i = 0; i < kPoints; ++i) {
        const double u = f.x[i] > 0.0 ? std::pow(f.x[i], 2.0 * b) : 0.0;
        const double r = 1.0 / (1.0 + a * u) - f.y[i];
        s += r * r;
    }
    return s;
}

}  // namespace

extern "C" int karma_umap_ab(double spread, double min_dist, double* a_out, double* b_out) {
    if (!a_out || !b_out || !(spread > 0.0) || !std::isfinite(spread) || !(min_dist >= 0.0) ||
        !std::isfinite(min_dist))
        return KARMA_ERR_ARG;
    Fit f;
    for (int i = 0; i < kPoints; ++i) {
        f.x[i] = (3.0 * spread) * (double)i / (double)(kPoints - 1);
        f.y[i] = f.x[i] < min_dist ? 1.0 : std::exp(-(f.x[i] - min_dist) / spread);
    }
    double a = 1.0, b = 1.0, lambda = 1e-3;
    double c = cost(f, a, b);
    for (int it = 0; it < 500; ++it) {
        // J^T J and J^T r of the residuals r_i = model(x_i) - y_i
        double jaa = 0.0, jab = 0.0, jbb = 0.0, ga = 0.0, gb = 0.0;
        for (int i = 0; i < kPoints; ++i) {
            if (!(f.x[i] > 0.0)) continue;  // the model is 1 at x = 0 whatever a and b are
            const double u = std::pow(f.x[i], 2.0 * b), den = 1.0 + a * u;
            const double r = 1.0 / den - f.y[i];
            const double da = -u / (den * den);
            const double db = -a * u * 2.0 * std::log(f.x[i]) / (den * den);
            jaa += da * da, jab += da * db, jbb += db * db;
            ga += da * r, gb += db * r;
        }
        bool moved = false;
        double step = 0.0;
        for (int tries = 0; tries < 40 && !moved; ++tries) {
            const double maa = jaa * (1.0 + lambda), mbb = jbb * (1.0 + lambda);
            const double det = maa * mbb - jab * jab;
            if (det != 0.0 && std::isfinite(det)) {
                const double sa = (-ga * mbb + gb * jab) / det, sb = (-gb * maa + ga * jab) / det;
                const double na = a + sa, nb = b + sb;
                const double nc = (na > 0.0 && nb > 0.0) ? cost(f, na, nb) : INFINITY;
                if (nc <= c) {
                    step = std::fabs(sa) / na + std::fabs(sb) / nb;
                    a = na, b = nb, c = nc;
                    lambda = lambda > 1e-12 ? lambda * 0.1 : lambda;
                    moved = true;
                    break;
                }
            }
            lambda *= 10.0;
        }
        if (!moved || step < 1e-14) break;
    }
    *a_out = a;
    *b_out = b;
    return KARMA_OK;
}
