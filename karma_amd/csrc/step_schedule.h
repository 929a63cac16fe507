// step_schedule.h — which stream each part of a deferred step goes to (step.hip
// run_deferred).  The whole assignment is one value computed by one pure
// function, so a change of what overlaps with what is a change here.  Host
// code only, no HIP; unit-tested without a GPU (tests/test_step_schedule_cpu.py,
// step_schedule_test.cpp).
#pragma once
#include <cstdint>

namespace karma {

constexpr int kMarkOne = 2;  // deferred batches on one main stream (SetsJob::launch positions)
constexpr int kMarkTwo = 4;  // deferred batches alternating two main streams (5, after the final kernel: 8-rank
                             // strong preview 0.196 against 0.188 ms with the binned classify)
constexpr int kMarkOneFlagged = 2;  // ... on flagged records too.  3 (at once, beside classify, which reads half the
                                    // bytes and is VALU-bound) measured 0.849 against 0.860 ms at config 3 (three
                                    // reps each; after classify 0.928, after the final kernel 0.911), but then
                                    // neither kernel's live time is its own (classify 0.65 ms live beside the
                                    // profile): not kept for 1 %, profiles/r06/measurements.md (r06h)
constexpr int64_t kAltMaxRecords = int64_t(1) << 27;  // batches below this alternate main streams

// The step's four streams (karma_step: main_s, alt_s, side_s, side_alt_s); run_deferred indexes by the value.
enum class StreamRole : int { kNone = 0, kMain = 1, kAlt = 2, kSide = 3, kSideAlt = 4 };

// Several processes: every deferred step's exchange and edge stage (all of the
// main communicator's operations) go to one exchange stream (see karma_step::xstream).
constexpr StreamRole kExchangeStream = StreamRole::kSideAlt;

// What run_deferred reads to place a step, and nothing else (aggregate: in this order).
struct ScheduleIn {
    int world = 1;          // processes of the communicator
    bool xstream = true;    // KARMA_STEP_XSTREAM
    bool one_comm = true;   // no distinct side communicator
    int streams = 0;        // KARMA_STEP_STREAMS: 1 / 2 main streams (0: by the batch's size)
    int64_t A = 0;          // records of the batch
    bool sequential = false;  // KARMA_STEP_SEQUENTIAL: every kernel alone on the chip
    bool flg = false;       // KARMA_STEP_FLAGGED records
    uint64_t seq = 0;       // the step's sequence number (from 1)
};

struct DeferredSchedule {
    bool two = false;    // batches alternate two main streams
    bool xs_on = false;  // the tail runs on the exchange stream
    int par = 0;         // which main stream, tail buffers and ev_tail this step uses
    StreamRole records = StreamRole::kMain;  // the records job (classify .. final kernel)
    StreamRole side = StreamRole::kSide;     // presence, column table, profile
    StreamRole tail = StreamRole::kMain;     // exchange, merge, edge stage, status kernel
    StreamRole fork = StreamRole::kNone;     // the records job's general-read branch (none: stays on its stream)
    bool single_stream = false;              // SetsOpts::single_stream
    int mark = kMarkOne;                     // SetsOpts::mark: where the side stream's profile may start
    int plan_zero = 0;                       // karma_step::plan_zero of the side stream
    // the profile is enqueued from inside the records job, at its mark, and
    // the job's next kernel waits until the side stream has passed the mark
    // (SetsOpts::at_mark): the profile is dispatched ahead of the final kernel
    bool profile_at_mark = false;
};

inline DeferredSchedule deferred_schedule(const ScheduleIn& in) {
    DeferredSchedule d;
    // Two batches in flight pay off only while one batch leaves the chip idle
    // between its short kernels: at config 3's size (308M records) two records
    // jobs side by side took 1.89 ms per batch against 1.23 ms one after the
    // other (they evict each other's partition runs from the caches); the
    // 8-rank strong preview (38.6M records) went 0.237 -> 0.199 ms.
    // several processes: two main streams only with the exchange stream
    // (the main communicator's operations then all go to it)
    d.two = (in.world == 1 || (in.xstream && !in.sequential)) &&
            (in.streams ? in.streams == 2 : in.A < kAltMaxRecords);
    // the exchange stream carries the tail: with two main streams, and with
    // one communicator also behind one main stream (it then holds every
    // collective of the step, the presence all-gather included)
    // (several processes only.  Emulated ranks keep the tail on the main
    // stream: the exchange stream's 8 more event calls per step cost more than
    // the overlap gains, 8-rank strong preview 0.200 / 0.204 against 0.193 /
    // 0.186 ms, same box)
    d.xs_on = !in.sequential && in.xstream && in.world > 1 && (d.two || in.one_comm);
    d.par = in.sequential || !d.two ? 0 : (int)(in.seq & 1);
    d.records = d.par ? StreamRole::kAlt : StreamRole::kMain;
    // with two main streams, the odd batches' presence, column table and
    // profile go to side_alt (unless it is busy as the exchange stream);
    // sequential: all on the records job's stream (the per-kernel timing pass)
    d.side = in.sequential ? d.records : d.par && !d.xs_on ? StreamRole::kSideAlt : StreamRole::kSide;
    d.tail = d.xs_on ? kExchangeStream : d.records;
    // the general-read branch: on the idle spare main stream with one main
    // stream; kept on the records job's stream with two (see karma_step::side_alt_s)
    d.single_stream = d.two;
    d.fork = d.two ? StreamRole::kNone : StreamRole::kAlt;
    // where the side stream's profile may start (SetsJob::launch): with one main
    // stream, after the code partition -- the profile's writes then share HBM
    // with the LDS-bound code reduce and final kernel instead of the next
    // batch's classify (config 3: 1.15 against 1.20-1.22 ms per step,
    // profiles/r04/measurements.md (ab_mark3)); with two, after the final kernel
    d.mark = d.two ? kMarkTwo : in.flg ? kMarkOneFlagged : kMarkOne;
    d.plan_zero = d.side == StreamRole::kSideAlt ? 1 : 0;
    // One process, one main stream: the profile and the final kernel become
    // ready within microseconds of each other on two queues, and a final kernel
    // dispatched first lets the next classify in beside the profile (0.85-0.99
    // against 0.79 ms per step at config 3).  The order is pinned instead of
    // raced.  (Several processes keep the host order of their collectives; two
    // main streams mark after the code reduce and want the overlap.)
    d.profile_at_mark = in.world == 1 && !in.sequential && !d.two;
    return d;
}

}  // namespace karma
