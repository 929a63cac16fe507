// flag.hip — {read id, contig} pairs -> KARMA_REC_FLAGGED words on the device
// (karma_records_flag), and the same words from read-sorted columns for the
// unsorted records job (graph.hip).
//
// Both kernels are pure streams: a lane takes kFlagPer consecutive records per
// round as 16-byte loads and stores their words as one 16-byte vector; a block
// tile is kFlagRounds rounds, all of a tile's loads issued before its first
// store; blocks stride over the tiles from a one-round grid.  Record i starts a
// read when i == 0 or read[i] != read[i - 1]: the predecessor of a lane's first
// record is the neighbouring lane's last one (a wave shuffle), that of a wave's
// first record one extra 4-byte load.  Checks (read ids decrease, contig id
// >= 2^31) and the read count go to a small control block the host reads after
// the stream synchronisation; nothing in a kernel traps.
#include <algorithm>

#include "flag_args.h"
#include "karma_internal.h"

using namespace karma;

namespace {

enum FlagCtrl : int { kFcOrder = 0, kFcRange, kFcReads, kFcWords };

// interleaved pairs, 16-byte aligned: two records per uint4
struct PairsSrc {
    const uint4* __restrict__ rec;
    static constexpr bool kOrder = true;
    __device__ __forceinline__ void load4(int64_t i, uint32_t (&rd)[kFlagPer], uint32_t (&cg)[kFlagPer]) const {
        const uint4 a = rec[i >> 1], b = rec[(i >> 1) + 1];
        rd[0] = a.x, cg[0] = a.y, rd[1] = a.z, cg[1] = a.w;
        rd[2] = b.x, cg[2] = b.y, rd[3] = b.z, cg[3] = b.w;
    }
    __device__ __forceinline__ uint32_t read(int64_t i) const {
        return reinterpret_cast<const uint32_t*>(rec)[2 * i];
    }
    __device__ __forceinline__ uint32_t contig(int64_t i) const {
        return reinterpret_cast<const uint32_t*>(rec)[2 * i + 1];
    }
};

// read ids and contigs as two columns sorted by read id, 16-byte aligned
struct ColumnsSrc {
    const uint32_t* __restrict__ rid;
    const uint32_t* __restrict__ cid;
    static constexpr bool kOrder = false;  // the sort's output
    __device__ __forceinline__ void load4(int64_t i, uint32_t (&rd)[kFlagPer], uint32_t (&cg)[kFlagPer]) const {
        const uint4 a = *reinterpret_cast<const uint4*>(rid + i), b = *reinterpret_cast<const uint4*>(cid + i);
        rd[0] = a.x, rd[1] = a.y, rd[2] = a.z, rd[3] = a.w;
        cg[0] = b.x, cg[1] = b.y, cg[2] = b.z, cg[3] = b.w;
    }
    __device__ __forceinline__ uint32_t read(int64_t i) const { return rid[i]; }
    __device__ __forceinline__ uint32_t contig(int64_t i) const { return cid[i]; }
};

struct FlagStats {
    unsigned starts = 0;
    bool bad_order = false, bad_range = false;
};

// One block tile.  FULL: every record of the tile exists (no bounds checks).
template <bool FULL, typename Src>
__device__ __forceinline__ void flag_tile(const Src& src, int64_t tile0, int64_t n, uint32_t* __restrict__ out,
                                          FlagStats& st) {
    const int lane = threadIdx.x & 63;
    const int64_t base = tile0 + (int64_t)threadIdx.x * kFlagPer;
    uint32_t rd[kFlagRounds][kFlagPer], cg[kFlagRounds][kFlagPer], pv[kFlagRounds];
#pragma unroll
    for (int r = 0; r < kFlagRounds; ++r) {
        const int64_t i0 = base + (int64_t)r * kFlagRound;
        if (FULL || i0 + kFlagPer <= n) {
            src.load4(i0, rd[r], cg[r]);
        } else {
#pragma unroll
            for (int k = 0; k < kFlagPer; ++k) {
                const bool ok = i0 + k < n;
                rd[r][k] = ok ? src.read(i0 + k) : 0u;
                cg[r][k] = ok ? src.contig(i0 + k) : 0u;
            }
        }
        // a wave's first record: its predecessor's read id by one 4-byte load
        pv[r] = 0;
        if (lane == 0 && i0 > 0 && (FULL || i0 < n)) pv[r] = src.read(i0 - 1);
    }
#pragma unroll
    for (int r = 0; r < kFlagRounds; ++r) {
        const int64_t i0 = base + (int64_t)r * kFlagRound;
        const uint32_t up = __shfl_up(rd[r][kFlagPer - 1], 1, 64);  // every lane takes part
        uint32_t prev = lane == 0 ? pv[r] : up;
        uint32_t w[kFlagPer];
#pragma unroll
        for (int k = 0; k < kFlagPer; ++k) {
            const int64_t i = i0 + k;
            const bool live = FULL || i < n;
            const bool first = i == 0 || rd[r][k] != prev;
            if (Src::kOrder) st.bad_order |= live && i > 0 && rd[r][k] < prev;
            st.bad_range |= live && (cg[r][k] >> 31);
            st.starts += live && first ? 1u : 0u;
            // an id >= 2^31 becomes 2^31 - 1: the word stays a contig no graph holds (n_contigs <= 2^24)
            w[k] = ((cg[r][k] >> 31) ? 0x7FFFFFFFu : cg[r][k]) | (first ? 0x80000000u : 0u);
            prev = rd[r][k];
        }
        if (FULL || i0 + kFlagPer <= n) {
            *reinterpret_cast<uint4*>(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kFlagPer; ++k)
                if (i0 + k < n) out[i0 + k] = w[k];
        }
    }
}

// ctrl (may be null: no checks reported, no count): kFcWords words, zeroed
template <typename Src>
__device__ __forceinline__ void flag_stream(const Src& src, int64_t n, uint32_t* __restrict__ out,
                                            unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned s_starts[kFlagThreads / 64];
    FlagStats st;
    const int64_t n_tiles = (n + kFlagTile - 1) / kFlagTile;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t tile0 = t * kFlagTile;
        if (tile0 + kFlagTile <= n) flag_tile<true>(src, tile0, n, out, st);
        else flag_tile<false>(src, tile0, n, out, st);
    }
    if (!ctrl) return;
    if (st.bad_order) ctrl[kFcOrder] = 1;
    if (st.bad_range) ctrl[kFcRange] = 1;
    unsigned s = st.starts;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) s_starts[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int w = 0; w < kFlagThreads / 64; ++w) tot += s_starts[w];
        if (tot) atomicAdd(ctrl + kFcReads, tot);
    }
}

__global__ __launch_bounds__(kFlagThreads) void flag_sorted_pairs_kernel(const uint4* __restrict__ rec, int64_t n,
                                                                         uint32_t* __restrict__ out,
                                                                         unsigned long long* __restrict__ ctrl) {
    flag_stream(PairsSrc{rec}, n, out, ctrl);
}

__global__ __launch_bounds__(kFlagThreads) void flag_sorted_columns_kernel(const uint32_t* __restrict__ rid,
                                                                           const uint32_t* __restrict__ cid, int64_t n,
                                                                           uint32_t* __restrict__ out,
                                                                           unsigned long long* __restrict__ ctrl) {
    flag_stream(ColumnsSrc{rid, cid}, n, out, ctrl);
}

template <typename K>
int flag_grid(karma_ctx* ctx, K kernel, int64_t n) {
    return resident_grid(ctx, reinterpret_cast<const void*>(kernel), kFlagThreads, 0, ceil_div(n, kFlagTile));
}

}  // namespace

int karma::flag_sorted_columns(karma_ctx* ctx, const uint32_t* rid, const uint32_t* cid, int64_t n, uint32_t* out,
                               unsigned long long* ctrl) {
    if (n <= 0) return KARMA_OK;
    KARMA_LAUNCH(ctx, "flag_sorted_columns", flag_sorted_columns_kernel, flag_grid(ctx, flag_sorted_columns_kernel, n),
                 kFlagThreads, 0, rid, cid, n, out, ctrl);
    return KARMA_OK;
}

extern "C" {

int karma_records_flag_tile(int* per_thread, int* per_wave, int* per_block) {
    KARMA_CHECK(per_thread && per_wave && per_block, KARMA_ERR_ARG, "karma_records_flag_tile: null out");
    *per_thread = kFlagPer;
    *per_wave = kFlagWave;
    *per_block = kFlagTile;
    return KARMA_OK;
}

int karma_records_flag(karma_ctx* ctx, const uint32_t* records, int64_t n, int rec_format, int is_device,
                       uint32_t* out, int out_is_device, int64_t* n_reads) {
    KARMA_TRY(ctx_begin(ctx));
    static_assert(KARMA_REC_SORTED == 0 && KARMA_REC_UNSORTED == 1, "flag_check_args takes the formats as 0 and 1");
    const FlagArgError bad = flag_check_args(records, n, rec_format, is_device, out, out_is_device);
    KARMA_CHECK(bad == kFlagArgsOk, KARMA_ERR_ARG, "%s", flag_arg_message(bad));
    if (n_reads) *n_reads = 0;
    if (n == 0) return KARMA_OK;

    // the kernels stream 16-byte vectors: host memory and pointers off a
    // 16-byte boundary go through an aligned temporary
    DevArray<uint2> own;
    DevArray<uint32_t> ownw;
    DevArray<unsigned long long> ctrl;
    const uint2* rec = reinterpret_cast<const uint2*>(records);
    if (!is_device || (reinterpret_cast<uintptr_t>(records) & 15)) {
        KARMA_TRY(own.alloc(ctx, n));
        KARMA_HIP(hipMemcpyAsync(own.ptr, records, n * 8, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                 ctx->stream));
        rec = own.ptr;
    }
    uint32_t* w = out;
    if (!out_is_device || (reinterpret_cast<uintptr_t>(out) & 15)) {
        KARMA_TRY(ownw.alloc(ctx, n));
        w = ownw.ptr;
    }
    KARMA_TRY(ctrl.alloc(ctx, kFcWords));
    KARMA_HIP(hipMemsetAsync(ctrl.ptr, 0, kFcWords * 8, ctx->stream));
    if (rec_format == KARMA_REC_SORTED) {
        KARMA_LAUNCH(ctx, "flag_sorted_pairs", flag_sorted_pairs_kernel, flag_grid(ctx, flag_sorted_pairs_kernel, n),
                     kFlagThreads, 0, reinterpret_cast<const uint4*>(rec), n, w, ctrl.ptr);
    } else {
        DevArray<uint32_t> rid, cid;
        KARMA_TRY(records_sorted_columns(ctx, rec, n, rid, cid));
        KARMA_TRY(flag_sorted_columns(ctx, rid.ptr, cid.ptr, n, w, ctrl.ptr));
    }
    unsigned long long* h = nullptr;
    KARMA_TRY(ctx_pinned(ctx, kFcWords * 8, reinterpret_cast<void**>(&h)));
    KARMA_HIP(hipMemcpyAsync(h, ctrl.ptr, kFcWords * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (w != out)
        KARMA_HIP(hipMemcpyAsync(out, w, n * 4, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                 ctx->stream));
    KARMA_HIP(hipStreamSynchronize(ctx->stream));
    KARMA_CHECK(!h[kFcOrder], KARMA_ERR_UNSORTED, "records are not grouped by read (read ids decrease)");
    KARMA_CHECK(!h[kFcRange], KARMA_ERR_ARG, "a record's contig index is >= 2^31 (flagged words hold ids below it)");
    if (n_reads) *n_reads = (int64_t)h[kFcReads];
    return KARMA_OK;
}

}  // extern "C"
