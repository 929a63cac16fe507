// code_part_test.cpp — code_part.h without a GPU: one partition block's
// bookkeeping driven flush by flush with adversarial and seeded histograms,
// every index checked against the sizes graph_sets.hip declares from the same
// header (make code_part_test; tests/test_code_part_cpu.py).
#include "code_part.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

using namespace karma;

static int checks = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        ++checks;                                                             \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

typedef std::vector<uint32_t> Hist;

// code_append_kernel<kMaxBc>'s arrays as it declares them
constexpr int NB = kMaxBc;
constexpr int kStage = (int)staged_bound(kAppendCap, NB);
constexpr int kVMax = kAppendCap / 8 + NB;
constexpr int kParentStage = kAppendCap + 8 * NB;  // the size before staged_bound
static_assert(kStage % 8 == 0 && kVMax >= staged_vectors(kAppendCap, NB), "");
static_assert(staged_bound(kAppendCap, 293) <= kParentStage && staged_bound(kAppendCap, 294) > kParentStage,
              "the earlier size held up to 293 buckets");
static_assert(staged_bound(kAppendCap, 391) == 17760 && staged_bound(kAppendCap, 512) == 19456 &&
                  staged_bound(kAppendCap, 300) == 16488,
              "the worst region sums by hand");
static_assert(staged_bound(kAppendCap, 512) <= kAppendCap + 14 * 512, "");
static_assert(staged_bound(100, 512) == 8 * 512 + 8 * 50, "fewer codes than two per bucket");

// One block of code_append_kernel over its flushes (each a per-bucket histogram;
// all but the last hold kAppendCap codes).  Every LDS and slice index the
// kernel forms is checked against `stage` (s16's size), kVMax and the block's
// slice.  Returns the most codes a flush staged; *over: some index left s16.
static uint32_t run_block(int nb, const std::vector<Hist>& flushes, int stage, bool* over) {
    std::vector<uint32_t> bh(nb, 0), pc(nb, 0), wr(nb, 0), rb(nb + 1, 0), toff(nb + 1), qoff(nb + 1);
    uint64_t items = 0;
    for (const Hist& h : flushes)
        for (int b = 0; b < nb; ++b) bh[b] += h[b], items += h[b];
    for (int b = 0; b < nb; ++b) rb[b + 1] = rb[b] + ((bh[b] + 7u) & ~7u);
    const int64_t need = append_need(items, nb);
    CHECK(rb[nb] <= need && need % 8 == 0);
    std::vector<uint8_t> written(rb[nb] / 8, 0);  // the slice's vectors, each stored once
    uint32_t worst = 0;
    *over = false;
    for (size_t f = 0; f < flushes.size(); ++f) {
        const Hist& h = flushes[f];
        const uint64_t n = std::accumulate(h.begin(), h.end(), uint64_t(0));
        CHECK(n <= (uint64_t)kAppendCap && (n == (uint64_t)kAppendCap || f + 1 == flushes.size()) && n > 0);
        const std::vector<uint32_t> pc0 = pc, wr0 = wr;
        const uint32_t staged = flush_scan(nb, h.data(), pc.data(), wr.data(), toff.data(), qoff.data());
        worst = std::max(worst, staged);
        CHECK(staged % 8 == 0 && (int64_t)staged <= staged_bound(kAppendCap, nb));
        CHECK((int64_t)qoff[nb] <= staged_vectors(kAppendCap, nb) && qoff[nb] <= (uint32_t)kVMax);
        if ((int)staged > stage) *over = true;
        for (int b = 0; b < nb; ++b) {
            const FlushBucket fb = flush_bucket(pc0[b], h[b]);
            CHECK(toff[b] % 8 == 0 && toff[b + 1] - toff[b] == fb.r8 && qoff[b + 1] - qoff[b] == fb.q);
            // pending codes at toff[b] + j (j < pc), new codes at cur[b] + rank (rank < h[b])
            const uint32_t cur = toff[b] + pc0[b];
            if (h[b]) {
                CHECK(h[b] - 1 < (1u << 16));  // the packed 16-bit ranks
                CHECK(cur + h[b] - 1 < toff[b + 1]);
                if ((int)(cur + h[b] - 1) >= stage) *over = true;
            }
            // full vectors: s16[toff + 8 k .. + 8) to the run at rb + wr0 + 8 k
            const uint32_t dlt = rb[b] + wr0[b] - toff[b];  // may wrap, as the kernel's does
            for (uint32_t k = 0; k < fb.q; ++k) {
                const uint32_t si = toff[b] + 8 * k, at = dlt + si;
                CHECK(si + 8 <= toff[b + 1] && at % 8 == 0 && at >= rb[b] && at + 8 <= rb[b + 1]);
                CHECK(!written[at / 8]);
                written[at / 8] = 1;
            }
            // the rest becomes the pending tail: one 16-byte read inside the region
            if (fb.rem) CHECK(toff[b] + (fb.tot & ~7u) + 8 <= toff[b + 1]);
            CHECK(pc[b] == fb.rem && pc[b] < 8 && wr[b] == wr0[b] + 8 * fb.q);
        }
    }
    for (int b = 0; b < nb; ++b) {  // the runs' last vectors; the counts agree with the classify's
        CHECK(wr[b] + pc[b] == bh[b]);
        if (pc[b]) {
            const uint32_t at = rb[b] + wr[b];
            CHECK(at + 8 == rb[b + 1] && !written[at / 8]);
            written[at / 8] = 1;
        } else {
            CHECK(rb[b] + wr[b] == rb[b + 1]);
        }
    }
    CHECK(std::all_of(written.begin(), written.end(), [](uint8_t w) { return w == 1; }));
    return worst;
}

// n codes over nb buckets: `base` each (given), the rest in whole eights to
// bucket `to` and a remainder of < 8 to the last bucket
static Hist top_up(Hist h, uint32_t n, int to) {
    const uint32_t have = std::accumulate(h.begin(), h.end(), 0u);
    CHECK(have <= n);
    h[to] += (n - have) & ~7u;
    h.back() += (n - have) & 7u;
    return h;
}

// The adversary: flush 1 leaves 7 pending codes in as many buckets as a full
// flush can (the pending codes of a block sum to 0 mod 8 after full flushes,
// so unless 8 divides nb one bucket keeps fewer), flush 2 brings every bucket
// the fewest codes that put its total at 1 (mod 8): 7 of padding each.
static std::vector<Hist> worst_case(int nb) {
    std::vector<Hist> fl;
    fl.push_back(top_up(Hist(nb, 7), kAppendCap, 0));
    Hist h2(nb);
    for (int b = 0; b < nb; ++b) h2[b] = (1u - fl[0][b]) & 7u;  // pc + h = 1 (mod 8)
    const uint32_t have = std::accumulate(h2.begin(), h2.end(), 0u);
    h2[0] += (kAppendCap - have) & ~7u;  // whole eights keep the residues
    fl.push_back(h2);
    return fl;
}

static void test_bound_direct() {
    // the bound is the maximum over every (pc, h) state, reached with pc = 7
    // and h = 2 (mod 8) everywhere, and not exceeded by any other residue choice
    for (int nb : {1, 2, 57, 129, 293, 294, 391, 512}) {
        for (int cap : {100, 4096, kCodeFill, kAppendCap}) {
            std::vector<uint32_t> pc(nb, 7), wr(nb, 0), toff(nb + 1), qoff(nb + 1);
            Hist h(nb, 0);
            int left = cap;
            for (int b = 0; b < nb && left >= 2; ++b) h[b] = 2, left -= 2;
            h[0] += left & ~7;
            CHECK((int64_t)flush_scan(nb, h.data(), pc.data(), wr.data(), toff.data(), qoff.data()) ==
                  staged_bound(cap, nb));
            std::mt19937 rng(nb * 7919 + cap);
            for (int it = 0; it < 300; ++it) {
                std::vector<uint32_t> p(nb);
                Hist g(nb, 0);
                for (int b = 0; b < nb; ++b) p[b] = it % 3 ? rng() % 8 : 7 - rng() % 2;
                int l = cap;
                for (int b = 0; b < nb && l > 0; ++b) {
                    const int x = std::min<int>(l, it % 2 ? rng() % 12 : 2 + 8 * (rng() % 2));
                    g[b] = x, l -= x;
                }
                g[rng() % nb] += l;
                std::fill(wr.begin(), wr.end(), 0);
                CHECK((int64_t)flush_scan(nb, g.data(), p.data(), wr.data(), toff.data(), qoff.data()) <=
                      staged_bound(cap, nb));
            }
        }
    }
}

static void test_blocks() {
    for (int nb : {129, 293, 294, 391, 512}) {
        bool over = false, over_parent = false;
        const std::vector<Hist> w = worst_case(nb);
        const uint32_t worst = run_block(nb, w, kStage, &over);
        CHECK(!over);
        // met (run_block checks it is never exceeded); at 129 buckets the one
        // bucket a full flush leaves without pending codes stages 8 fewer
        CHECK((int64_t)worst == staged_bound(kAppendCap, nb) - (nb == 129 ? 8 : 0));
        CHECK(run_block(nb, w, kParentStage, &over_parent) == worst);
        CHECK(over_parent == (nb >= 294));  // the earlier size: overrun from 294 buckets on
        std::printf("nb %d: worst staged %u, bound %lld, declared %d, earlier size %d%s\n", nb, worst,
                    (long long)staged_bound(kAppendCap, nb), kStage, kParentStage,
                    over_parent ? " (overrun)" : "");
        // every residue of the per-bucket counts over three flushes, one bucket
        // holding everything, buckets with no code, a short last flush
        std::vector<std::vector<Hist>> seqs;
        {
            std::vector<Hist> s;
            for (int f = 0; f < 3; ++f) {
                Hist h(nb);
                for (int b = 0; b < nb; ++b) h[b] = (uint32_t)((b + 3 * f) % 8);
                s.push_back(top_up(h, kAppendCap, (f * 5) % nb));
            }
            seqs.push_back(s);
            Hist one(nb, 0);
            one[nb / 2] = kAppendCap;
            Hist tail(nb, 0);
            tail[nb / 2] = 1;
            seqs.push_back({one, one, tail});
            seqs.push_back({one});
            seqs.push_back({tail});
        }
        std::mt19937 rng(nb);
        for (int it = 0; it < 40; ++it) {
            std::vector<Hist> s;
            const int nf = 1 + rng() % 4;
            for (int f = 0; f < nf; ++f) {
                const uint32_t n = f + 1 < nf ? kAppendCap : 1 + rng() % kAppendCap;
                Hist h(nb, 0);
                const int live = it % 4 == 0 ? nb : 1 + rng() % nb;  // buckets that get codes
                if (it % 2) {
                    for (uint32_t i = 0; i < n; ++i) ++h[rng() % live];
                } else {  // small counts of every residue, the rest to one bucket
                    uint32_t l = n;
                    for (int b = 0; b < live && l; ++b) {
                        const uint32_t x = std::min<uint32_t>(l, rng() % 17);
                        h[b] = x, l -= x;
                    }
                    h[rng() % live] += l;
                }
                s.push_back(h);
            }
            seqs.push_back(s);
        }
        for (const auto& s : seqs) {
            run_block(nb, s, kStage, &over);
            CHECK(!over);
        }
    }
}

// partition_kernel<CodeStream>: a flush's padded runs fit sorted[], a block's
// flushes fit the stream slice and directory rows part_need gives it
static void test_part_need() {
    std::mt19937 rng(5);
    for (int nb : {1, 57, 64, 65, 128}) {
        for (uint64_t items : {uint64_t(0), uint64_t(1), uint64_t(kCodeFill - 1), uint64_t(kCodeFill),
                               uint64_t(kCodeFill + 1), uint64_t(2 * kCodeFill), uint64_t(2 * kCodeFill + 1)}) {
            for (int mode = 0; mode < 3; ++mode) {
                int64_t outs, rows;
                part_need(items, kCodeFill, nb, kCodePad, &outs, &rows);
                CHECK(rows == (int64_t)((items + kCodeFill - 1) / kCodeFill) && outs % kCodePad == 0);
                int64_t used = 0, nrow = 0;
                for (uint64_t base = 0; base < items; base += kCodeFill, ++nrow) {
                    const uint32_t n = (uint32_t)std::min<uint64_t>(kCodeFill, items - base);
                    Hist h(nb, 0);
                    if (mode == 0) h[nb - 1] = n;  // one bucket: ranks up to n - 1
                    else if (mode == 1) {          // as many counts of 1 (mod 8) as n gives
                        uint32_t l = n;
                        for (int b = 0; b < nb && l; ++b) h[b] = 1, --l;
                        h[0] += l & ~7u, h[nb - 1] += l & 7u;
                    } else for (uint32_t i = 0; i < n; ++i) ++h[rng() % nb];
                    uint32_t c2 = 0;
                    for (int b = 0; b < nb; ++b) {
                        CHECK(h[b] == 0 || h[b] - 1 < (1u << 16));
                        c2 += (h[b] + (kCodePad - 1)) & ~(uint32_t)(kCodePad - 1);
                    }
                    CHECK(c2 <= (uint32_t)(kCodeFill + kNarrowBc * (kCodePad - 1)));  // sorted[]
                    used += c2;
                }
                CHECK(nrow == rows && used <= outs);
            }
        }
    }
}

static void test_constants() {
    CHECK(reduce_split(0) == 1 && reduce_split(1) == kCrSmax && reduce_split(8) == 64 && reduce_split(9) == 57);
    CHECK(reduce_split(511) == 2 && reduce_split(512) == 1 && reduce_split(513) == 1 && reduce_split(1 << 20) == 1);
    for (int64_t R = 1; R < 2000; ++R) {
        const int S = reduce_split(R);
        CHECK(S >= 1 && S <= kCrSmax && (S == 1 || R * S < kCrPieces + R));
    }
    CHECK(append_need(0, 391) % 8 == 0 && append_need(0, 391) >= 391 * 7);
    CHECK(append_need(12345, 129) >= 12345 + 129 * 7 && append_need(12345, 129) < 12345 + 129 * 7 + 8);
    CHECK(kRoundVecs == 1024 && kAppendCap % kPT == 0 && kCodeFill % kPT == 0 && kAppendCap < (1 << 16));
    CHECK((kMaxListsPerBlock & (kMaxListsPerBlock - 1)) == 0);
}

int main() {
    test_constants();
    test_bound_direct();
    test_blocks();
    test_part_need();
    std::printf("ok (%d checks)\n", checks);
    return 0;
}
