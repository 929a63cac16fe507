// sets_ctrl.h — the layout of a records job's control block (graph_sets.hip
// SetsJob; karma_step's kernels read it and its status kernel zeroes it).
// Offsets in 8-byte words.  Host code only, no HIP; unit-tested without a GPU
// (tests/test_sets_ctrl_cpu.py, sets_ctrl_test.cpp).
#pragma once
#include <cstdint>

namespace karma {

// flags: 4 ints at CtrlLayout::flags
enum CtrlFlag : int {
    kFlagOrder = 0,      // records not grouped by read (read ids decrease)
    kFlagContigRange,    // a record's contig index >= n_contigs
    kFlagPairCap,        // a chunk's pair list was full: rerun with room for every pair
    kFlagPartition,      // code partition: block counts disagree with the classify histogram
    kCtrlFlags
};
// counters: unsigned words at CtrlLayout::counters (room for 8)
enum CtrlCounter : int {
    kCtrBigReads = 0,    // reads of more than 8 records
    kCtrCodeFlushes,     // the code partition's flushes
    kCtrPairFlushes,     // the pair partition's flushes
    kCtrRelabel,         // set: this pass is skipped, a relabelled rerun follows
    kCtrVote,            // classify's vote for the relabel (a caller's zeroed block: no probe)
    kCtrlCounters
};

// One block, cleared by one memset (or kept zero by the step's status kernel):
//   flags[4] | counters[5 of 8] | pairs per bucket[B+1] | their exclusive scan dst[B+1]
//   (dst[B]: the list's length) | overflow bytes[B] | split counts[n_split]
// -- read back by one copy up to here --
//   | items per partition block[2 n_pblk] (codes, then pairs) | the final kernel's look-back words[B]
struct CtrlLayout {
    static constexpr int64_t flags = 0;
    static constexpr int64_t counters = 2;
    static constexpr int64_t n_per = 6;
    // the wide path's block: the flags and the first 4 counters (it flushes and relabels nothing)
    static constexpr int64_t small_words = 4;
    int64_t dst, ovf, split_loc;
    int64_t readback;  // words the host reads back
    int64_t blk_items, lb;
    int64_t total;
    int64_t list_len;  // dst[B]

    CtrlLayout(int64_t B, int64_t n_split, int64_t n_pblk)
        : dst(n_per + (B + 1)),
          ovf(dst + (B + 1)),
          split_loc(ovf + (B + 7) / 8),
          readback(split_loc + n_split),
          blk_items(readback),
          lb(blk_items + 2 * n_pblk),
          total(lb + B),
          list_len(dst + B) {}
};
static_assert(CtrlLayout::counters * 8 == kCtrlFlags * 4, "the counters follow the flags");
static_assert((CtrlLayout::n_per - CtrlLayout::counters) * 2 >= kCtrlCounters, "the counters fit ahead of the counts");

}  // namespace karma
