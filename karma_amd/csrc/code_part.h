// code_part.h — the arithmetic of the records graph's code-partition path
// (graph_sets.hip: partition_kernel<CodeStream>, code_append_kernel,
// code_reduce_kernel through stream_runs): its constants, a block's output
// need, the per-flush bookkeeping of code_append_kernel and the size its
// staging array must have.  Plain C++, no HIP header: graph_sets.hip includes
// it (constexpr functions are callable from kernels), and it is unit-tested
// without a GPU (tests/test_code_part_cpu.py, code_part_test.cpp).
#pragma once
#include <cstdint>

namespace karma {

constexpr int kPT = 512;                // partition threads (several blocks per CU overlap their phases)
constexpr int kMaxListsPerBlock = 128;  // chunk lists per partition block, at most (a power of 2)
constexpr int kCodeFill = 8192;         // codes per flush of partition_kernel<CodeStream> (32 KB of LDS)
constexpr int kCodePad = 8;             // a run of u16 codes is padded to 16 bytes
constexpr int kMaxBc = 512;             // code buckets
// partition_kernel<CodeStream> up to kNarrowBc code buckets (n_contigs <= 2^19,
// 3 blocks per CU); code_append_kernel from kAppendMinBc on
constexpr int kNarrowBc = 128;
constexpr int kAppendMinBc = 129;
static_assert(kAppendMinBc == kNarrowBc + 1, "every bucket count has exactly one code-partition kernel");
// codes per flush of code_append_kernel: 8192 codes write ~20 codes per run
// at the weak-scaled config 3 instead of ~10 (0.26-0.27 vs 0.29 ms); 12288:
// ~30 per run, weak 8-rank preview 1.412 -> 1.397 ms; 16384 leaves one block
// per CU: 1.60 ms
constexpr int kAppendCap = 12288;
constexpr int kCrSmax = 64;     // code reduce: at most this many pieces per run
constexpr int kCrPieces = 512;  // code reduce: split runs into pieces only while a block has < 512 (per-piece cost dominates: 2048 -> 512 took the 8-rank strong reduce 48.6 -> 26.2 us, weak 126 -> 81 us)
constexpr int kCgShift = 18;    // a code bucket gets one reduce group per 2^18 records it may hold
constexpr int kWin = 16;        // stream_runs: windows of 64 vectors in flight before they are counted
constexpr int kRoundVecs = 64 * kWin;  // 16-byte vectors of one stream_runs round of a wave

// A partition block's items (blk_items, summed by the producers), flushes
// (every flush but the last holds cap items) and an output bound (items + <
// pad per run): the bases of block b are these sums over blocks < b, so each
// block derives its own directory rows and stream slice (no atomics, no plan
// launch).
constexpr void part_need(uint64_t items, int cap, int nb, int pad, int64_t* outs, int64_t* rows) {
    *rows = ((int64_t)items + cap - 1) / cap;
    *outs = ((int64_t)items + *rows * (int64_t)nb * (pad - 1) + pad - 1) / pad * pad;
}

// code_append_kernel: one run per (block, bucket), padded once
constexpr int64_t append_need(uint64_t items, int nb) {
    return ((int64_t)items + (int64_t)nb * (kCodePad - 1) + (kCodePad - 1)) / kCodePad * kCodePad;
}

// code_reduce_kernel: a group's R directory rows are read as R * S runs
constexpr int reduce_split(int64_t R) {
    if (R <= 0) return 1;
    const int64_t s = (kCrPieces + R - 1) / R;
    return (int)(s < 1 ? 1 : s > kCrSmax ? kCrSmax : s);
}

// ---- one flush of code_append_kernel ----------------------------------------------
// Bucket b enters a flush with pc[b] < 8 pending codes (the tail of its run
// that did not fill a 16-byte vector yet) and h[b] new ones.  Its region of the
// staging array starts 8-aligned and holds the pending codes, then the new
// ones; its full vectors go to the run, the rest is the next pending tail.
struct FlushBucket {
    uint32_t tot;  // pending + new codes
    uint32_t r8;   // codes of the region (tot rounded up to 8)
    uint32_t q;    // full vectors written by this flush
    uint32_t rem;  // the next pending tail (< 8)
};
constexpr FlushBucket flush_bucket(uint32_t pc, uint32_t h) {
    const uint32_t tot = pc + h;
    return FlushBucket{tot, (tot + 7u) & ~7u, tot >> 3, tot & 7u};
}

// The scan over the buckets (the kernel's wave 0 runs it 64 buckets at a
// time): region starts toff[nb + 1] and vectors before each bucket
// qoff[nb + 1]; then pc and wr move on as at the flush's end.  Returns the
// staged codes toff[nb].
inline uint32_t flush_scan(int nb, const uint32_t* h, uint32_t* pc, uint32_t* wr, uint32_t* toff, uint32_t* qoff) {
    uint32_t c8 = 0, cq = 0;
    for (int b = 0; b < nb; ++b) {
        const FlushBucket f = flush_bucket(pc[b], h[b]);
        toff[b] = c8;
        qoff[b] = cq;
        c8 += f.r8;
        cq += f.q;
        pc[b] = f.rem;
        wr[b] += f.tot & ~7u;
    }
    toff[nb] = c8;
    qoff[nb] = cq;
    return c8;
}

// The most codes one flush stages (the regions' sum toff[nb]), over every
// pc[b] <= 7 and every h with sum h <= cap.  Bucket b's region is
// roundup8(pc + h); for a given h the worst pc gives
//   f(h) = 8 * floor((h + 14) / 8):  8 for h <= 1, 16 for 2 <= h <= 9, ...
// (pc = 7 and h = 2 (mod 8): 7 pending, h new and 7 of padding).  f rises by 8
// at h = 2 and then once per 8 codes, so the best use of cap codes is 2 in
// every bucket (16 each) and the rest in whole eights:
//   cap >= 2 nb:  16 nb + 8 floor((cap - 2 nb) / 8)   (<= cap + 14 nb)
//   cap <  2 nb:  8 nb + 8 floor(cap / 2)             (floor(cap / 2) buckets of 2)
// The parent of this header sized the array cap + 8 nb: too small from 294
// buckets on at cap = 12288.
constexpr int64_t staged_bound(int64_t cap, int64_t nb) {
    return cap >= 2 * nb ? 16 * nb + ((cap - 2 * nb) & ~int64_t(7)) : 8 * nb + 8 * (cap / 2);
}
// full vectors of one flush: sum of floor(tot / 8) <= (cap + 7 nb) / 8
constexpr int64_t staged_vectors(int64_t cap, int64_t nb) { return (cap + 7 * nb) / 8; }

}  // namespace karma
