// flag_args.h — karma_records_flag's tile constants and argument checks: a pure
// host header (no HIP), shared by flag.hip and flag_args_test.cpp.
#pragma once

#include <cstdint>

namespace karma {

// The sorted kernels' tile.  A lane takes kFlagPer consecutive records per
// round (two 16-byte loads of pairs, one 16-byte store of words), a wave
// 64 * kFlagPer, a block kFlagRounds rounds of kFlagThreads * kFlagPer records.
constexpr int kFlagThreads = 256;
constexpr int kFlagPer = 4;
constexpr int kFlagRounds = 4;
constexpr int kFlagWave = 64 * kFlagPer;               // records per wave and round
constexpr int kFlagRound = kFlagThreads * kFlagPer;    // records per block and round
constexpr int kFlagTile = kFlagRound * kFlagRounds;    // records per block tile

constexpr int64_t kFlagMaxSorted = int64_t(1) << 40;    // karma_graph_records' own limit
constexpr int64_t kFlagMaxUnsorted = int64_t(1) << 31;  // the radix sort's

enum FlagArgError : int {
    kFlagArgsOk = 0,
    kFlagArgsNull,      // a null pointer with records to convert, or n_records < 0
    kFlagArgsFormat,    // rec_format is neither SORTED (0) nor UNSORTED (1)
    kFlagArgsTooMany,   // n_records past the format's limit
    kFlagArgsAlign,     // records or out not 4-byte aligned
    kFlagArgsOverlap,   // records and out share bytes
};

// [a, a + na) and [b, b + nb) share a byte (empty ranges share nothing)
inline bool flag_ranges_overlap(uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) {
    if (!na || !nb) return false;
    return a < b ? b - a < na : a - b < nb;
}

// rec_format: 0 sorted, 1 unsorted (KARMA_REC_SORTED / _UNSORTED).  The ranges
// are compared only when both lie in the same address space.
inline FlagArgError flag_check_args(const void* records, int64_t n, int rec_format, int is_device, const void* out,
                                    int out_is_device) {
    if (n < 0 || (n > 0 && (!records || !out))) return kFlagArgsNull;
    if (rec_format != 0 && rec_format != 1) return kFlagArgsFormat;
    if (n >= (rec_format == 0 ? kFlagMaxSorted : kFlagMaxUnsorted)) return kFlagArgsTooMany;
    const uintptr_t r = reinterpret_cast<uintptr_t>(records), o = reinterpret_cast<uintptr_t>(out);
    if (n > 0 && ((r & 3) || (o & 3))) return kFlagArgsAlign;
    if (!is_device == !out_is_device && flag_ranges_overlap(r, (uint64_t)n * 8, o, (uint64_t)n * 4))
        return kFlagArgsOverlap;
    return kFlagArgsOk;
}

inline const char* flag_arg_message(FlagArgError e) {
    switch (e) {
        case kFlagArgsNull: return "karma_records_flag: bad arguments";
        case kFlagArgsFormat: return "karma_records_flag: rec_format must be KARMA_REC_SORTED or KARMA_REC_UNSORTED";
        case kFlagArgsTooMany: return "karma_records_flag: too many records";
        case kFlagArgsAlign: return "karma_records_flag: records and out must be 4-byte aligned";
        case kFlagArgsOverlap: return "karma_records_flag: records and out overlap";
        default: return "";
    }
}

}  // namespace karma
