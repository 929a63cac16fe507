// umap_args_test.cpp — the UMAP entries' argument checks (umap_args.h) and the
// defined functions (umap_math.h) on the host, built with AddressSanitizer +
// UBSan (make umap_args_test; tests/test_umap_args_cpu.py).  No GPU code.
#include <cstdio>
#include <cstring>
#include <vector>

#include "umap_args.h"
#include "umap_math.h"

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

static double from_bits(uint64_t b) {
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}
static uint64_t to_bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

// {argument bits, result bits} of the numpy model (tests/umap_reference.py): 0, +-1, the clamps and beyond them,
// results around the smallest normal, random arguments; klog at 1, powers of two, both sides of sqrt(1/2), the
// smallest subnormal, the smallest normal, the largest finite value
static const uint64_t kExpCases[][2] = {
    {0x0000000000000000ull, 0x3ff0000000000000ull}, {0x3ff0000000000000ull, 0x4005bf0a8b14576aull},
    {0xbff0000000000000ull, 0x3fd78b56362cef38ull}, {0x4086280000000000ull, 0x7fdd422d2be5dc9bull},
    {0x4086300000000000ull, 0x7fdd422d2be5dc9bull}, {0xc087480000000000ull, 0x0000000000000001ull},
    {0xc087500000000000ull, 0x0000000000000001ull}, {0xc087440000000000ull, 0x0000000000000001ull},
    {0x3fe0000000000000ull, 0x3ffa61298e1e069cull}, {0xbfd62e42fefa39f0ull, 0x3fe6a09e667f3bccull},
    {0x40562e42feba39efull, 0x47efffffdffffff5ull}, {0xc086232bdd7abcd2ull, 0x001000000000007cull},
    {0x01a56e1fc2f8f359ull, 0x3ff0000000000000ull}, {0xc042c00000000000ull, 0x3c8dd5c566301ec8ull},
    {0x40308cdecb7e76c0ull, 0x416d62837056d049ull}, {0x4083b531829649e0ull, 0x78cc87d401c159bbull},
    {0xc07f22d31de7f34eull, 0x1303784af1b2a319ull}, {0x4083a0dfb1e080f6ull, 0x78920072ddf00c75ull},
    {0xc07076f9b8ba3148ull, 0x282ebe7bc6564562ull}, {0xc05ad5f33e79d758ull, 0x3641977d310140bdull},
};
static const uint64_t kLogCases[][2] = {
    {0x3ff0000000000000ull, 0x0000000000000000ull}, {0x4000000000000000ull, 0x3fe62e42fefa39efull},
    {0x3fe0000000000000ull, 0xbfe62e42fefa39efull}, {0x3fe6a09e667f3bcdull, 0xbfd62e42fefa39eeull},
    {0x3fe6a09e667f3bccull, 0xbfd62e42fefa39f1ull}, {0x3fe6a09e667f3bceull, 0xbfd62e42fefa39ebull},
    {0x0000000000000001ull, 0xc0874385446d71c3ull}, {0x0010000000000000ull, 0xc086232bdd7abcd2ull},
    {0x7fefffffffffffffull, 0x40862e42fefa39efull}, {0x4024000000000000ull, 0x40026bb1bbb55516ull},
    {0x3f50624dd2f1a9fcull, 0xc01ba18a998fffa0ull}, {0x4008000000000000ull, 0x3ff193ea7aad030bull},
    {0x42e364b316297b37ull, 0x40406297dc03a890ull}, {0x3f1ddc7d4b5e6dd3ull, 0xc0222901146c9a04ull},
    {0x4061d01f3f727a14ull, 0x4013d664c4218810ull}, {0x3bacaa154fc17c7dull, 0xc0479f3e4c37b68aull},
    {0x4237d2616cd14a13ull, 0x403959ef824e8f10ull}, {0x4046ac579fd64f37ull, 0x400e83c023de4ec0ull},
};

int main() {
    static_assert(kKnnKMax == 64 && kUmapDimMax == 16 && kUmapMaxDim == 16, "umap_arg_message names the limits");

    // ---- the defined functions, bit for bit the model's
    for (const auto& c : kExpCases) EXPECT(to_bits(kexp(from_bits(c[0]))) == c[1]);
    for (const auto& c : kLogCases) EXPECT(to_bits(klog(from_bits(c[0]))) == c[1]);
    EXPECT(splitmix64(12345) == 0xf36cf1164265dd51ull);
    EXPECT(to_bits(umap_init_value(42, 2 * 2 + 1)) == 0x401d754f9e32e844ull);  // y[2, 1] of a 3 x 2 start
    EXPECT(umap_clip4(5.0) == 4.0 && umap_clip4(-4.5) == -4.0 && umap_clip4(0.25) == 0.25);

    // ---- karma_umap_graph
    std::vector<int32_t> idx(64, 0), ind(256);
    std::vector<double> dist(64, 0.0), wts(256), sg(8), rh(8);
    std::vector<int64_t> ptr(9);
    int64_t nnz = 0;
    const int64_t cap = 2 * 8 * 3;
    auto graph = [&](const void* i, const void* d, int64_t n, int k, const void* p, const void* x, const void* w,
                     int64_t c, const void* z, const void* s, const void* r) {
        return umap_graph_check_args(i, d, n, k, p, x, w, c, z, s, r);
    };
    const void *I = idx.data(), *D = dist.data(), *P = ptr.data(), *X = ind.data(), *W = wts.data(), *Z = &nnz,
               *S = sg.data(), *R = rh.data();
    EXPECT(graph(I, D, 8, 3, P, X, W, cap, Z, S, R) == kUmapArgsOk);
    EXPECT(graph(I, D, 8, 3, P, X, W, cap, Z, nullptr, nullptr) == kUmapArgsOk);  // sigma and rho are optional
    EXPECT(graph(I, D, 2, 2, P, X, W, 8, Z, S, R) == kUmapArgsOk);                // the smallest case
    EXPECT(graph(I, D, 1, 2, P, X, W, cap, Z, S, R) == kUmapArgsShape);
    EXPECT(graph(I, D, 0, 2, P, X, W, cap, Z, S, R) == kUmapArgsShape);
    EXPECT(graph(I, D, kKnnMaxRows, 2, P, X, W, cap, Z, S, R) == kUmapArgsShape);
    EXPECT(graph(I, D, 8, 1, P, X, W, cap, Z, S, R) == kUmapArgsK);
    EXPECT(graph(I, D, 8, 9, P, X, W, 1000, Z, S, R) == kUmapArgsK);  // k > n
    EXPECT(graph(I, D, 1000, 65, P, X, W, 1 << 20, Z, S, R) == kUmapArgsK);
    EXPECT(graph(I, D, 1000, 64, P, X, W, 128000, Z, S, R) == kUmapArgsOk);
    EXPECT(graph(nullptr, D, 8, 3, P, X, W, cap, Z, S, R) == kUmapArgsNull);
    EXPECT(graph(I, nullptr, 8, 3, P, X, W, cap, Z, S, R) == kUmapArgsNull);
    EXPECT(graph(I, D, 8, 3, nullptr, X, W, cap, Z, S, R) == kUmapArgsNull);
    EXPECT(graph(I, D, 8, 3, P, nullptr, W, cap, Z, S, R) == kUmapArgsNull);
    EXPECT(graph(I, D, 8, 3, P, X, nullptr, cap, Z, S, R) == kUmapArgsNull);
    EXPECT(graph(I, D, 8, 3, P, X, W, cap, nullptr, S, R) == kUmapArgsNull);
    EXPECT(graph(I, (const char*)D + 4, 8, 3, P, X, W, cap, Z, S, R) == kUmapArgsAlign);
    EXPECT(graph((const char*)I + 2, D, 8, 3, P, X, W, cap, Z, S, R) == kUmapArgsAlign);
    EXPECT(graph(I, D, 8, 3, (const char*)P + 4, X, W, cap, Z, S, R) == kUmapArgsAlign);
    EXPECT(graph(I, D, 8, 3, P, X, W, cap, Z, (const char*)S + 4, R) == kUmapArgsAlign);
    EXPECT(graph(I, D, 8, 3, P, X, W, cap, Z, S, (const char*)R + 1) == kUmapArgsAlign);
    EXPECT(graph(idx.data() + 1, D, 8, 3, P, ind.data() + 1, W, cap, Z, S, R) == kUmapArgsOk);  // int32: 4 bytes
    EXPECT(graph(I, D, 8, 3, P, X, W, cap - 1, Z, S, R) == kUmapArgsCap);
    EXPECT(graph(I, D, int64_t(1) << 25, 64, P, X, W, INT64_MAX, Z, S, R) == kUmapArgsBytes);  // 2 n k = 2^32
    EXPECT(graph(I, D, (int64_t(1) << 25) - 1, 64, P, X, W, INT64_MAX, Z, S, R) == kUmapArgsOk);
    EXPECT(graph(nullptr, D, 8, 1, P, X, W, 0, Z, S, R) == kUmapArgsK);  // the first failing check names the error
    // the lists' contents
    for (int e = 0; e < 24; ++e) idx[e] = e % 8;
    EXPECT(umap_check_lists(idx.data(), 8, 3) == kUmapArgsOk);
    idx[23] = 8;
    EXPECT(umap_check_lists(idx.data(), 8, 3) == kUmapArgsIndex);
    idx[23] = -1;
    EXPECT(umap_check_lists(idx.data(), 8, 3) == kUmapArgsIndex);

    // ---- karma_umap_layout
    std::vector<double> y(8 * 16);
    auto layout = [&](const void* p, const void* x, const void* w, int64_t n, int64_t z, int dim, double a, double b,
                      int epochs, int rate, double gamma, double alpha, const void* yy) {
        return umap_layout_check_args(p, x, w, n, z, dim, a, b, epochs, rate, gamma, alpha, yy);
    };
    const void* Y = y.data();
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsOk);
    EXPECT(layout(P, nullptr, nullptr, 8, 0, 1, 1.5, 0.9, 1, 0, 1.0, 1.0, Y) == kUmapArgsOk);  // an empty graph
    EXPECT(layout(P, X, W, 8, 20, 16, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsOk);
    EXPECT(layout(P, X, W, 1, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsShape);
    EXPECT(layout(P, X, W, kKnnMaxRows, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsShape);
    EXPECT(layout(P, X, W, 8, -1, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsNnz);
    EXPECT(layout(P, X, W, 8, 20, 0, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsDim);
    EXPECT(layout(P, X, W, 8, 20, 17, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsDim);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 0, 5, 1.0, 1.0, Y) == kUmapArgsEpochs);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 10, -1, 1.0, 1.0, Y) == kUmapArgsRate);
    EXPECT(layout(P, X, W, 8, 20, 2, NAN, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsParam);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, INFINITY, 10, 5, 1.0, 1.0, Y) == kUmapArgsParam);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, NAN, 1.0, Y) == kUmapArgsParam);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, -INFINITY, Y) == kUmapArgsParam);
    EXPECT(layout(nullptr, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsNull);
    EXPECT(layout(P, nullptr, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsNull);
    EXPECT(layout(P, X, nullptr, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsNull);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, nullptr) == kUmapArgsNull);
    EXPECT(layout((const char*)P + 4, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsAlign);
    EXPECT(layout(P, (const char*)X + 2, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsAlign);
    EXPECT(layout(P, X, (const char*)W + 4, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsAlign);
    EXPECT(layout(P, X, W, 8, 20, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, (const char*)Y + 4) == kUmapArgsAlign);
    EXPECT(layout(P, X, W, 8, INT64_MAX / 16, 2, 1.5, 0.9, 10, 5, 1.0, 1.0, Y) == kUmapArgsBytes);
    // the CSR contents: a path 0 - 1 - 2 with an empty row 3
    const int64_t good_ptr[5] = {0, 1, 3, 4, 4};
    const int32_t good_ind[4] = {1, 0, 2, 1};
    const double good_w[4] = {1.0, 1.0, 0.5, 0.5};
    EXPECT(umap_check_csr(good_ptr, good_ind, good_w, 4, 4) == kUmapArgsOk);
    EXPECT(umap_check_csr(good_ptr, good_ind, good_w, 4, 3) == kUmapArgsIndptr);  // does not end at nnz
    const int64_t dec_ptr[5] = {0, 3, 1, 4, 4}, off_ptr[5] = {1, 1, 3, 4, 4};
    EXPECT(umap_check_csr(dec_ptr, good_ind, good_w, 4, 4) == kUmapArgsIndptr);
    EXPECT(umap_check_csr(off_ptr, good_ind, good_w, 4, 4) == kUmapArgsIndptr);
    const int32_t high_ind[4] = {1, 0, 4, 1}, neg_ind[4] = {1, -1, 2, 1};
    EXPECT(umap_check_csr(good_ptr, high_ind, good_w, 4, 4) == kUmapArgsColumn);
    EXPECT(umap_check_csr(good_ptr, neg_ind, good_w, 4, 4) == kUmapArgsColumn);
    const double zero_w[4] = {1.0, 1.0, 0.0, 0.5}, nan_w[4] = {1.0, NAN, 0.5, 0.5};
    const double inf_w[4] = {INFINITY, 1.0, 0.5, 0.5};
    EXPECT(umap_check_csr(good_ptr, good_ind, zero_w, 4, 4) == kUmapArgsWeight);
    EXPECT(umap_check_csr(good_ptr, good_ind, nan_w, 4, 4) == kUmapArgsWeight);
    EXPECT(umap_check_csr(good_ptr, good_ind, inf_w, 4, 4) == kUmapArgsWeight);

    for (int e = kUmapArgsShape; e <= kUmapArgsWeight; ++e) EXPECT(umap_arg_message((UmapArgError)e)[0] != 0);
    EXPECT(umap_arg_message(kUmapArgsOk)[0] == 0);

    // ---- one vertex's epoch on the host: a two-point graph, one attraction; the move is along the line and inward
    {
        const int64_t ip[3] = {0, 1, 2};
        const int32_t ix[2] = {1, 0};
        const double eps[2] = {1.0, 1.0};
        double eons[2] = {0.0, 0.0}, eonns[2] = {INFINITY, INFINITY};
        uint32_t t[2] = {0, 0};
        const double y_old[4] = {0.0, 0.0, 3.0, 4.0};
        double y_new[4] = {};
        for (int64_t i = 0; i < 2; ++i)
            umap_vertex_epoch<2>(i, 2, ip, ix, eps, eons, eonns, t, y_old, y_new, 0, 1.0, 1.5, 0.9, 1.0, 0, 7);
        EXPECT(y_new[0] > 0.0 && y_new[1] > 0.0 && y_new[2] < 3.0 && y_new[3] < 4.0);
        EXPECT(eons[0] == 1.0 && eons[1] == 1.0 && t[0] == 0);
    }

    if (g_failed) return 1;
    std::printf("ok (%d cases)\n", g_cases);
    return 0;
}
