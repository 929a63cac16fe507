// spectral_args_test.cpp — the spectral entries' argument checks and round bound
// (spectral_args.h) and the small dense problems (spectral_small.h) on the
// host, built with AddressSanitizer + UBSan (make spectral_args_test;
// tests/test_spectral_args_cpu.py).  No GPU code.
#include <cstdio>
#include <vector>

#include "spectral_args.h"
#include "spectral_small.h"

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

// a fixed generator for the matrices below
static uint64_t g_state = 0x243F6A8885A308D3ull;
static double next_unit() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * 0x1p-53 - 0.5;
}

// |a v - v diag(w)| and |v^T v - I|, largest entries
static double eig_error(const std::vector<double>& a, int p, const double* w, const double* v) {
    double worst = 0.0;
    for (int i = 0; i < p; ++i)
        for (int k = 0; k < p; ++k) {
            double av = 0.0, vv = 0.0;
            for (int j = 0; j < p; ++j) {
                av += a[i * p + j] * v[j * p + k];
                vv += v[j * p + i] * v[j * p + k];
            }
            worst = std::fmax(worst, std::fabs(av - w[k] * v[i * p + k]));
            worst = std::fmax(worst, std::fabs(vv - (i == k ? 1.0 : 0.0)));
        }
    return worst;
}

int main() {
    static_assert(kSpectralBasisMax == kSpectralBlockMax + 1 && kUmapDimMax + kSpectralGuard <= kSpectralBlockMax,
                  "a block of dim + guard columns and the trivial vector fit the small problems");
    static_assert(kSpectralColsMax == 32 && kSpectralDegree >= 2, "spectral_arg_message names the limits");

    // ---- argument checks
    std::vector<int64_t> ptr(9, 0);
    std::vector<int32_t> ind(32, 0), comp(8);
    std::vector<double> wts(32, 1.0), y(8 * 16), x(8 * 32), out(8 * 32);
    int64_t count = 0, info[4] = {};
    const void *P = ptr.data(), *X = ind.data(), *W = wts.data(), *Y = y.data(), *C = comp.data();
    EXPECT(components_check_args(P, X, 8, 20, C, &count) == kSpectralArgsOk);
    EXPECT(components_check_args(P, X, 1, 0, C, &count) == kSpectralArgsOk);  // one vertex is a graph
    EXPECT(components_check_args(P, nullptr, 8, 0, C, &count) == kSpectralArgsOk);
    EXPECT(components_check_args(P, X, 0, 20, C, &count) == kSpectralArgsShape);
    EXPECT(components_check_args(P, X, kKnnMaxRows, 20, C, &count) == kSpectralArgsShape);
    EXPECT(components_check_args(P, X, 8, -1, C, &count) == kSpectralArgsNnz);
    EXPECT(components_check_args(nullptr, X, 8, 20, C, &count) == kSpectralArgsNull);
    EXPECT(components_check_args(P, nullptr, 8, 20, C, &count) == kSpectralArgsNull);
    EXPECT(components_check_args(P, X, 8, 20, nullptr, &count) == kSpectralArgsNull);
    EXPECT(components_check_args(P, X, 8, 20, C, nullptr) == kSpectralArgsNull);
    EXPECT(components_check_args((const char*)P + 4, X, 8, 20, C, &count) == kSpectralArgsAlign);
    EXPECT(components_check_args(P, (const char*)X + 2, 8, 20, C, &count) == kSpectralArgsAlign);
    EXPECT(components_check_args(P, X, 8, 20, (const char*)C + 1, &count) == kSpectralArgsAlign);
    EXPECT(components_check_args(P, X, 8, INT64_MAX / 16, C, &count) == kSpectralArgsBytes);

    EXPECT(apply_check_args(P, X, W, 8, 20, x.data(), 32, out.data()) == kSpectralArgsOk);
    EXPECT(apply_check_args(P, X, W, 8, 20, x.data(), 1, out.data()) == kSpectralArgsOk);
    EXPECT(apply_check_args(P, X, W, 1, 20, x.data(), 1, out.data()) == kSpectralArgsShape);
    EXPECT(apply_check_args(P, X, W, 8, 20, x.data(), 0, out.data()) == kSpectralArgsCols);
    EXPECT(apply_check_args(P, X, W, 8, 20, x.data(), 33, out.data()) == kSpectralArgsCols);
    EXPECT(apply_check_args(P, X, nullptr, 8, 20, x.data(), 3, out.data()) == kSpectralArgsNull);
    EXPECT(apply_check_args(P, X, W, 8, 20, nullptr, 3, out.data()) == kSpectralArgsNull);
    EXPECT(apply_check_args(P, X, W, 8, 20, x.data(), 3, nullptr) == kSpectralArgsNull);
    EXPECT(apply_check_args(P, X, (const char*)W + 4, 8, 20, x.data(), 3, out.data()) == kSpectralArgsAlign);
    EXPECT(apply_check_args(P, X, W, 8, 20, (const char*)x.data() + 4, 3, out.data()) == kSpectralArgsAlign);

    auto solve = [&](const void* p, const void* xx, const void* w, int64_t n, int64_t nnz, int dim, double tol,
                     int outer, const void* yy, const void* v, const void* l, const void* r, const void* c,
                     const void* inf) {
        return spectral_check_args(p, xx, w, n, nnz, dim, tol, outer, yy, v, l, r, c, inf);
    };
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsOk);
    EXPECT(solve(P, X, W, 8, 20, 16, 1e-4, 1, Y, nullptr, nullptr, nullptr, nullptr, info) == kSpectralArgsOk);
    EXPECT(solve(P, nullptr, nullptr, 8, 0, 1, 1e-4, 1, Y, nullptr, nullptr, nullptr, nullptr, info) ==
           kSpectralArgsOk);  // an empty graph: n components
    EXPECT(solve(P, X, W, 1, 20, 2, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsShape);
    EXPECT(solve(P, X, W, 8, -1, 2, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsNnz);
    EXPECT(solve(P, X, W, 8, 20, 0, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsDim);
    EXPECT(solve(P, X, W, 8, 20, 17, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsDim);
    EXPECT(solve(P, X, W, 8, 20, 2, 0.0, 100, Y, Y, Y, Y, C, info) == kSpectralArgsTol);
    EXPECT(solve(P, X, W, 8, 20, 2, -1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsTol);
    EXPECT(solve(P, X, W, 8, 20, 2, NAN, 100, Y, Y, Y, Y, C, info) == kSpectralArgsTol);
    EXPECT(solve(P, X, W, 8, 20, 2, INFINITY, 100, Y, Y, Y, Y, C, info) == kSpectralArgsTol);
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 0, Y, Y, Y, Y, C, info) == kSpectralArgsOuter);
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 100, nullptr, Y, Y, Y, C, info) == kSpectralArgsNull);
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 100, Y, Y, Y, Y, C, nullptr) == kSpectralArgsNull);
    EXPECT(solve(P, X, nullptr, 8, 20, 2, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsNull);
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 100, (const char*)Y + 4, Y, Y, Y, C, info) == kSpectralArgsAlign);
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 100, Y, Y, (const char*)Y + 4, Y, C, info) == kSpectralArgsAlign);
    EXPECT(solve(P, X, W, 8, 20, 2, 1e-4, 100, Y, Y, Y, Y, (const char*)C + 2, info) == kSpectralArgsAlign);
    EXPECT(solve(P, X, W, kKnnMaxRows - 1, 20, 16, 1e-4, 100, Y, Y, Y, Y, C, info) == kSpectralArgsBytes);
    for (int e = kSpectralArgsShape; e <= kSpectralArgsBytes; ++e)
        EXPECT(spectral_arg_message((SpectralArgError)e)[0] != 0);
    EXPECT(spectral_arg_message(kSpectralArgsOk)[0] == 0);

    // the structure of a graph without weights: a path 0 - 1 - 2 and an empty row
    const int64_t good_ptr[5] = {0, 1, 3, 4, 4}, dec_ptr[5] = {0, 3, 1, 4, 4};
    const int32_t good_ind[4] = {1, 0, 2, 1}, high_ind[4] = {1, 0, 4, 1};
    const double good_w[4] = {1.0, 1.0, 0.5, 0.5}, zero_w[4] = {1.0, 0.0, 0.5, 0.5};
    EXPECT(spectral_check_csr(good_ptr, good_ind, nullptr, 4, 4) == kUmapArgsOk);
    EXPECT(spectral_check_csr(good_ptr, good_ind, good_w, 4, 4) == kUmapArgsOk);
    EXPECT(spectral_check_csr(good_ptr, good_ind, nullptr, 4, 3) == kUmapArgsIndptr);
    EXPECT(spectral_check_csr(dec_ptr, good_ind, nullptr, 4, 4) == kUmapArgsIndptr);
    EXPECT(spectral_check_csr(good_ptr, high_ind, nullptr, 4, 4) == kUmapArgsColumn);
    EXPECT(spectral_check_csr(good_ptr, good_ind, zero_w, 4, 4) == kUmapArgsWeight);

    // ---- the round bound
    EXPECT(components_rounds_max(1) == 1 && components_rounds_max(2) == 3 && components_rounds_max(3) == 5);
    EXPECT(components_rounds_max(1024) == 21 && components_rounds_max(1025) == 23);
    EXPECT(components_rounds_max(kKnnMaxRows - 1) == 63);

    // ---- Jacobi: random symmetric matrices at every size, a matrix with repeated eigenvalues, a rank-deficient Gram
    for (int p = 1; p <= kSpectralBasisMax; ++p) {
        std::vector<double> a((size_t)p * p), work, w((size_t)p), v((size_t)p * p);
        for (int i = 0; i < p; ++i)
            for (int j = i; j < p; ++j) a[i * p + j] = a[j * p + i] = next_unit();
        work = a;
        EXPECT(spectral_jacobi(work.data(), p, w.data(), v.data()) < kSpectralSweepsMax);
        EXPECT(eig_error(a, p, w.data(), v.data()) < 1e-13 * p);
        for (int i = 1; i < p; ++i) EXPECT(w[i - 1] >= w[i]);
    }
    {
        const int p = 6;  // I + e e^T: eigenvalues 7, 1, 1, 1, 1, 1
        std::vector<double> a(p * p, 1.0), work, w(p), v(p * p);
        for (int i = 0; i < p; ++i) a[i * p + i] = 2.0;
        work = a;
        spectral_jacobi(work.data(), p, w.data(), v.data());
        EXPECT(std::fabs(w[0] - 7.0) < 1e-13);
        for (int i = 1; i < p; ++i) EXPECT(std::fabs(w[i] - 1.0) < 1e-13);
        EXPECT(eig_error(a, p, w.data(), v.data()) < 1e-13);
    }

    // ---- orth and ritz on an explicit basis: 5 vertices, u and p = 6 columns of which at most 4 are independent of u
    {
        const int s = 5, p = 6, PB = p + 1;
        std::vector<double> b((size_t)s * PB), sm((size_t)s * s), g((size_t)PB * PB), w((size_t)PB * p);
        // a symmetric operator with u = e / sqrt(5) as eigenvector of eigenvalue 1: sm = u u^T + r (I - u u^T) r' ...
        // simply: the normalised operator of the complete graph with unit weights, S = (J - I) / 4
        for (int i = 0; i < s; ++i)
            for (int j = 0; j < s; ++j) sm[i * s + j] = i == j ? 0.0 : 0.25;
        for (int i = 0; i < s; ++i) {
            b[i * PB] = 1.0 / std::sqrt(5.0);
            for (int k = 1; k < PB; ++k) b[i * PB + k] = next_unit();
        }
        auto gram = [&](const std::vector<double>& l, const std::vector<double>& r, std::vector<double>& o) {
            for (int i = 0; i < PB; ++i)
                for (int j = 0; j < PB; ++j) {
                    double t = 0.0;
                    for (int q = 0; q < s; ++q) t += l[q * PB + i] * r[q * PB + j];
                    o[i * PB + j] = t;
                }
        };
        gram(b, b, g);
        EXPECT(spectral_orth(g.data(), PB, w.data()) == s - 1);  // the fifth and sixth columns are dependent
        std::vector<double> q((size_t)s * PB, 0.0), sq((size_t)s * PB, 0.0), g2((size_t)PB * PB), h((size_t)PB * PB);
        for (int i = 0; i < s; ++i) {
            q[i * PB] = b[i * PB];
            for (int c = 0; c < p; ++c)
                for (int k = 0; k < PB; ++k) q[i * PB + 1 + c] += b[i * PB + k] * w[k * p + c];
        }
        for (int i = 0; i < s; ++i)
            for (int c = 0; c < PB; ++c)
                for (int j = 0; j < s; ++j) sq[i * PB + c] += sm[i * s + j] * q[j * PB + c];
        gram(q, q, g2);
        gram(q, sq, h);
        for (int c = 1; c <= s - 1; ++c) {
            EXPECT(std::fabs(g2[c * PB + c] - 1.0) < 1e-9 && std::fabs(g2[c]) < 1e-9);  // unit, orthogonal to u
        }
        EXPECT(g2[5 * PB + 5] == 0.0 && g2[6 * PB + 6] == 0.0);  // the dropped directions are zero columns
        std::vector<double> cm((size_t)PB * p), theta((size_t)p);
        EXPECT(spectral_ritz(g2.data(), h.data(), PB, cm.data(), theta.data()) == s - 1);
        for (int c = 0; c < s - 1; ++c) EXPECT(std::fabs(theta[c] + 0.25) < 1e-12);  // (J - I) / 4 off u: -1/4
        EXPECT(theta[4] == kSpectralNoRitz && theta[5] == kSpectralNoRitz);
        for (int k = 0; k < PB; ++k) EXPECT(cm[k * p + 4] == 0.0 && cm[k * p + 5] == 0.0);
    }
    {
        // a Gram matrix of zeros but u: nothing to keep, nothing read out of bounds
        const int PB = kSpectralBasisMax, p = PB - 1;
        std::vector<double> g((size_t)PB * PB, 0.0), w((size_t)PB * p), theta((size_t)p);
        g[0] = 1.0;
        EXPECT(spectral_orth(g.data(), PB, w.data()) == 0);
        EXPECT(spectral_ritz(g.data(), g.data(), PB, w.data(), theta.data()) == 0);
        g[0] = 0.0;
        EXPECT(spectral_orth(g.data(), PB, w.data()) == 0);
        // the identity at full size: every column kept
        for (int i = 0; i < PB; ++i) g[i * PB + i] = 1.0;
        EXPECT(spectral_orth(g.data(), PB, w.data()) == p);
        EXPECT(spectral_ritz(g.data(), g.data(), PB, w.data(), theta.data()) == p);
        for (int c = 0; c < p; ++c) EXPECT(std::fabs(theta[c] - 1.0) < 1e-14);
    }

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
