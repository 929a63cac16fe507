// spectral_small.h — the small dense problems of karma_umap_spectral, one per
// graph component and outer round, on the host: a cyclic Jacobi eigensolver, a
// Cholesky factorisation that drops dependent columns, and the two steps built
// on them (the orthonormalising transform of a filtered block, and the
// Rayleigh-Ritz step).  A pure host header (no HIP), shared by spectral.hip and
// spectral_args_test.cpp.  All matrices are row-major; P = p + 1 <= 33: index 0
// of a P-sized basis is the component's trivial vector u = sqrt(d) / |sqrt(d)|.
#pragma once

#include <cmath>
#include <cstdint>

namespace karma {

constexpr int kSpectralBlockMax = 32;             // columns of a block (p)
constexpr int kSpectralBasisMax = kSpectralBlockMax + 1;  // with the trivial vector (P)
constexpr int kSpectralSweepsMax = 64;
constexpr double kSpectralOrthDrop = 1e-11;  // relative pivot below which a filtered column counts as dependent
constexpr double kSpectralRitzDrop = 1e-8;   // the same for the (near-orthonormal) Ritz basis
constexpr double kSpectralNoRitz = -2.0;     // theta of a null direction (below every eigenvalue of S)

// Eigenvalues (descending, in w[p]) and eigenvectors (column k of v, v[i * p +
// k]) of the symmetric p x p matrix a, which is destroyed.  Cyclic Jacobi: a
// rotation is skipped once |a_ij| <= 2^-58 |a|_F, a sweep without a rotation
// ends the loop.  Returns the sweeps run (kSpectralSweepsMax: not settled).
inline int spectral_jacobi(double* a, int p, double* w, double* v) {
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) v[i * p + j] = i == j ? 1.0 : 0.0;
    double norm2 = 0.0;
    for (int i = 0; i < p * p; ++i) norm2 += a[i] * a[i];
    const double small = std::ldexp(std::sqrt(norm2), -58);
    int sweeps = 0;
    for (; sweeps < kSpectralSweepsMax; ++sweeps) {
        bool rotated = false;
        for (int i = 0; i < p - 1; ++i)
            for (int j = i + 1; j < p; ++j) {
                const double aij = a[i * p + j];
                if (!(std::fabs(aij) > small)) continue;
                rotated = true;
                const double th = (a[j * p + j] - a[i * p + i]) / (2.0 * aij);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < p; ++k) {  // columns i and j
                    const double ki = a[k * p + i], kj = a[k * p + j];
                    a[k * p + i] = c * ki - s * kj;
                    a[k * p + j] = s * ki + c * kj;
                }
                for (int k = 0; k < p; ++k) {  // rows i and j
                    const double ik = a[i * p + k], jk = a[j * p + k];
                    a[i * p + k] = c * ik - s * jk;
                    a[j * p + k] = s * ik + c * jk;
                }
                a[i * p + j] = 0.0;
                a[j * p + i] = 0.0;
                for (int k = 0; k < p; ++k) {
                    const double ki = v[k * p + i], kj = v[k * p + j];
                    v[k * p + i] = c * ki - s * kj;
                    v[k * p + j] = s * ki + c * kj;
                }
            }
        if (!rotated) break;
    }
    for (int i = 0; i < p; ++i) w[i] = a[i * p + i];
    for (int i = 1; i < p; ++i)  // insertion sort, descending, stable; p <= 33
        for (int j = i; j > 0 && w[j] > w[j - 1]; --j) {
            const double t = w[j];
            w[j] = w[j - 1];
            w[j - 1] = t;
            for (int k = 0; k < p; ++k) {
                const double u = v[k * p + j];
                v[k * p + j] = v[k * p + j - 1];
                v[k * p + j - 1] = u;
            }
        }
    return sweeps;
}

// The inverse m (q x q, lower triangular, row-major with stride kSpectralBasisMax)
// of the Cholesky factor of g (P x P) restricted to the columns it keeps: column j
// is dropped where g_jj <= 0 or its pivot falls to drop * g_jj or below (it lies
// in the span of the columns before it).  act[0 .. q) names the kept columns in
// order; returns q.
inline int spectral_chol_inverse(const double* g, int P, double drop, int* act, double* m) {
    constexpr int S = kSpectralBasisMax;
    double l[S * S];
    int q = 0;
    for (int j = 0; j < P; ++j) {
        const double gjj = g[j * P + j];
        if (!(gjj > 0.0) || !std::isfinite(gjj)) continue;
        double row[S];
        double piv = gjj;
        for (int k = 0; k < q; ++k) {  // l[j, k] against the kept columns so far
            double s = g[j * P + act[k]];
            for (int t = 0; t < k; ++t) s -= row[t] * l[k * S + t];
            row[k] = s / l[k * S + k];
            piv -= row[k] * row[k];
        }
        if (!(piv > drop * gjj)) continue;
        for (int k = 0; k < q; ++k) l[q * S + k] = row[k];
        l[q * S + q] = std::sqrt(piv);
        act[q++] = j;
    }
    for (int i = 0; i < q; ++i) {  // m = l^-1 by forward substitution, column by column
        for (int j = 0; j < q; ++j) m[i * S + j] = 0.0;
    }
    for (int j = 0; j < q; ++j)
        for (int i = j; i < q; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int t = j; t < i; ++t) s -= l[i * S + t] * m[t * S + j];
            m[i * S + j] = s / l[i * S + i];
        }
    return q;
}

// Step one of a round.  g = [u, Y]^T [u, Y] (P x P).  w (P x p): [u, Y] w has
// orthonormal columns that span Y's part outside u, column c belonging to Y's
// column c; a column that depends on those before it (a component with fewer
// than p + 1 vertices has such) becomes a zero column.  Returns the columns kept.
inline int spectral_orth(const double* g, int P, double* w) {
    constexpr int S = kSpectralBasisMax;
    const int p = P - 1;
    int act[S];
    double m[S * S];
    for (int i = 0; i < P * p; ++i) w[i] = 0.0;
    const int q = spectral_chol_inverse(g, P, kSpectralOrthDrop, act, m);
    if (q == 0 || act[0] != 0) return 0;  // u itself is missing: nothing to deflate against
    for (int jc = 1; jc < q; ++jc)
        for (int kc = 0; kc <= jc; ++kc) w[act[kc] * p + (act[jc] - 1)] = m[jc * S + kc];
    return q - 1;
}

// Step two.  g = [u, Q]^T [u, Q] and h = [u, Q]^T [u, S Q] (both P x P; h's
// column 0 is not read: S u = u).  c (P x p): the columns of [u, Q] c are the
// Ritz vectors of S on the span of Q outside u, orthonormal in g, by descending
// Ritz value theta[0 .. q); columns q .. p are zero and theta there is
// kSpectralNoRitz.  Returns q.
inline int spectral_ritz(const double* g, const double* h, int P, double* c, double* theta) {
    constexpr int S = kSpectralBasisMax;
    const int p = P - 1;
    int act[S];
    double m[S * S], hc[S * S], t1[S * S], hs[S * S], z[S * S], w[S];
    for (int i = 0; i < P * p; ++i) c[i] = 0.0;
    for (int i = 0; i < p; ++i) theta[i] = kSpectralNoRitz;
    const int qq = spectral_chol_inverse(g, P, kSpectralRitzDrop, act, m);
    if (qq < 2 || act[0] != 0) return 0;
    // the symmetrised operator on the kept columns; row and column 0 from g (S u = u)
    for (int a = 0; a < qq; ++a)
        for (int b = 0; b < qq; ++b) {
            const int i = act[a], j = act[b];
            hc[a * S + b] = (i == 0 || j == 0) ? g[i * P + j] : 0.5 * (h[i * P + j] + h[j * P + i]);
        }
    for (int a = 0; a < qq; ++a)  // t1 = m hc
        for (int b = 0; b < qq; ++b) {
            double s = 0.0;
            for (int k = 0; k <= a; ++k) s += m[a * S + k] * hc[k * S + b];
            t1[a * S + b] = s;
        }
    const int q = qq - 1;
    for (int a = 1; a < qq; ++a)  // hs = (t1 m^T) without the trivial direction
        for (int b = 1; b < qq; ++b) {
            double s = 0.0;
            for (int k = 0; k <= b; ++k) s += t1[a * S + k] * m[b * S + k];
            hs[(a - 1) * q + (b - 1)] = s;
        }
    for (int a = 0; a < q; ++a)
        for (int b = a + 1; b < q; ++b) hs[a * q + b] = hs[b * q + a] = 0.5 * (hs[a * q + b] + hs[b * q + a]);
    spectral_jacobi(hs, q, w, z);
    for (int col = 0; col < q; ++col) {
        theta[col] = w[col];
        for (int k = 0; k < qq; ++k) {  // c = m^T[:, 1:] z
            double s = 0.0;
            for (int l = (k > 1 ? k : 1); l < qq; ++l) s += m[l * S + k] * z[(l - 1) * q + col];
            c[act[k] * p + col] = s;
        }
    }
    return q;
}

}  // namespace karma
