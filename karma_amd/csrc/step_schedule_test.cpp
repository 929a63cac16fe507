// Host unit test of step_schedule.h (no GPU): hand-written rows of the
// deferred step's stream assignment, and its invariants over every
// combination of the inputs.  Built by `make -C karma_amd/csrc
// step_schedule_test`, run by tests/test_step_schedule_cpu.py.  Exit status
// 0 = every case passed.
#include <cstdio>
#include <initializer_list>

#include "step_schedule.h"

using namespace karma;

namespace {
int g_bad = 0, g_cases = 0;

#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++g_bad;                                               \
        }                                                          \
    } while (0)

constexpr int64_t kSmall = (int64_t(1) << 27) - 1, kLarge = int64_t(1) << 27;
constexpr StreamRole M = StreamRole::kMain, A = StreamRole::kAlt, S = StreamRole::kSide, SA = StreamRole::kSideAlt,
                     N = StreamRole::kNone;

DeferredSchedule at(int world, bool xstream, bool one_comm, int streams, int64_t records, bool sequential, bool flg,
                    uint64_t seq) {
    ScheduleIn in;
    in.world = world;
    in.xstream = xstream;
    in.one_comm = one_comm;
    in.streams = streams;
    in.A = records;
    in.sequential = sequential;
    in.flg = flg;
    in.seq = seq;
    return deferred_schedule(in);
}

// the rows of the step as it stood before the schedule was a value (streams = 0)
void rows() {
    {  // one process, small batch, odd step
        const DeferredSchedule d = at(1, true, true, 0, kSmall, false, false, 1);
        EXPECT(d.two && !d.xs_on && d.par == 1 && d.records == A && d.side == SA && d.tail == A && d.fork == N &&
               d.single_stream && d.mark == 4 && d.plan_zero == 1);
    }
    {  // ... even step
        const DeferredSchedule d = at(1, true, true, 0, kSmall, false, false, 2);
        EXPECT(d.two && !d.xs_on && d.par == 0 && d.records == M && d.side == S && d.tail == M && d.fork == N &&
               d.mark == 4 && d.plan_zero == 0);
    }
    for (int flg = 0; flg < 2; ++flg)  // one process, large batch
        for (uint64_t seq = 1; seq <= 2; ++seq) {
            const DeferredSchedule d = at(1, true, true, 0, kLarge, false, flg, seq);
            EXPECT(!d.two && !d.xs_on && d.par == 0 && d.records == M && d.side == S && d.tail == M && d.fork == A &&
                   !d.single_stream && d.mark == 2 && d.plan_zero == 0);
        }
    for (uint64_t seq = 1; seq <= 2; ++seq) {  // one process, sequential, small batch
        const DeferredSchedule d = at(1, true, true, 0, kSmall, true, false, seq);
        EXPECT(d.two && !d.xs_on && d.par == 0 && d.records == M && d.side == M && d.tail == M);
    }
    {  // two processes, exchange stream, one communicator, small batch, odd step
        const DeferredSchedule d = at(2, true, true, 0, kSmall, false, false, 1);
        EXPECT(d.two && d.xs_on && d.records == A && d.side == S && d.tail == SA && d.plan_zero == 0);
    }
    {  // ... large batch
        const DeferredSchedule d = at(2, true, true, 0, kLarge, false, false, 1);
        EXPECT(!d.two && d.xs_on && d.records == M && d.tail == SA && d.fork == A);
    }
    {  // two processes, exchange stream allowed, side communicator, large batch
        const DeferredSchedule d = at(2, true, false, 0, kLarge, false, false, 1);
        EXPECT(!d.two && !d.xs_on && d.tail == M);
    }
    for (int one_comm = 0; one_comm < 2; ++one_comm)  // two processes, no exchange stream
        for (int64_t records : {kSmall, kLarge}) {
            const DeferredSchedule d = at(2, false, one_comm, 0, records, false, false, 1);
            EXPECT(!d.two && !d.xs_on && d.par == 0);
        }
    {  // two processes, sequential
        const DeferredSchedule d = at(2, true, true, 0, kSmall, true, false, 1);
        EXPECT(!d.two && !d.xs_on && d.side == M);
    }
    // KARMA_STEP_STREAMS overrides the batch size
    EXPECT(!at(1, true, true, 1, kSmall, false, false, 1).two);
    EXPECT(at(1, true, true, 2, kLarge, false, false, 1).two);
}

void invariants() {
    for (int world = 1; world <= 2; ++world)
    for (int xstream = 0; xstream < 2; ++xstream)
    for (int one_comm = 0; one_comm < 2; ++one_comm)
    for (int streams = 0; streams <= 2; ++streams)
    for (int64_t records : {kSmall, kLarge})
    for (int sequential = 0; sequential < 2; ++sequential)
    for (int flg = 0; flg < 2; ++flg)
    for (uint64_t seq = 1; seq <= 2; ++seq) {
        const DeferredSchedule d = at(world, xstream, one_comm, streams, records, sequential, flg, seq);
        ++g_cases;
        const int bad0 = g_bad;
        if (d.xs_on) EXPECT(world > 1 && d.tail == SA && d.side == S);
        if (!d.two) EXPECT(d.par == 0 && d.fork == A);
        if (d.two) EXPECT(d.single_stream && d.fork == N);
        if (sequential) EXPECT(d.par == 0 && d.side == d.records);
        EXPECT(d.tail == d.records || d.tail == SA);
        if (!sequential) EXPECT(d.side != d.records);
        if (g_bad != bad0)
            std::printf("  at world %d xstream %d one_comm %d streams %d A %lld sequential %d flg %d seq %llu\n", world,
                        xstream, one_comm, streams, (long long)records, sequential, flg, (unsigned long long)seq);
    }
    EXPECT(g_cases == 384);
}
}  // namespace

int main() {
    rows();
    invariants();
    std::printf("%s (%d cases, %d failures)\n", g_bad ? "FAILED" : "ok", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
