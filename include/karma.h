/*
 * karma.h — C ABI of libkarma_hip.so, the MI355X (gfx950) implementation of
 * lmfaber/karma's k-mer profile + shared-read graph hot path.
 *
 * Plain C types only (pointers + sizes); no torch / HIP types in signatures
 * (streams are passed as void*).  Every function returns an int status
 * (KARMA_OK = 0, negative = error; message via karma_last_error()).
 *
 * Reference interfaces replaced (file:line under lmfaber/karma):
 *   karma_contigs_*, karma_kmer_*   KmerClustering.__calc_kmer_profile   karma/kmer.py:199-264
 *                                   (__extract_kmers :146-179, __kmers_of_seq :181-197,
 *                                    __count_kmer_occurence :56-92, fill_array_for_contig :108-122,
 *                                    is_palindrome :46-54)
 *   karma_graph_records             ReadGraph.from_contigs               karma/read_graph.py:19-50
 *                                   + Contig readsets                    karma/contig.py:4-35
 *                                   and ReadGraph.update_graph           karma/read_graph.py:192-221
 *   karma_graph_eq                  ReadGraph.from_equivalence_classes   karma/read_graph.py:61-148
 *   karma_pairs_merge{,_runs} /     (new) multi-GPU edge merge, SURVEY.md §8(e)
 *   _split / _totals
 *   karma_edges_*                   the normalised weight (s/|A| + s/|B|)/2  read_graph.py:39-42, :128-130
 *   karma_synth_*                   (new) deterministic synthetic inputs, SURVEY.md §8(d)
 *   karma_fasta_*                   read_fasta_file                      karma/karma.py:40-61
 *   karma_eq_*                      eq_classes.txt parse                 karma/read_graph.py:75-92
 *   karma_sam_*                     Contig readsets from SAM lines       karma/contig.py:24,34, hisat2.py:49-53
 *   karma_adj_*                     graph consumers: unconnected nodes, node weights, edge_list
 *                                   karma/read_graph.py:150-190, :315-357
 *   karma_adj_cross_sums            --rearrange subcluster connections  karma/karma.py:103-118
 *
 * The reference is pure Python and has no FFI; INTEGRATION.md shows the ctypes
 * binding (karma_amd/_lib.py) that the Python classes mirroring the reference
 * API (karma_amd/kmer.py, read_graph.py, contig.py) use.
 */
#ifndef KARMA_H
#define KARMA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define KARMA_OK 0
#define KARMA_ERR_ARG (-1)       /* invalid argument / unsupported size                       */
#define KARMA_ERR_KMER (-2)      /* unsupported k (supported: 1..8 and "5p6")                 */
#define KARMA_ERR_HIP (-3)       /* HIP runtime error (no device, launch failure, ...)        */
#define KARMA_ERR_OOM (-4)       /* device allocation failed                                  */
#define KARMA_ERR_ZERO_DIV (-5)  /* non-zero count over a zero normaliser (ZeroDivisionError) */
#define KARMA_ERR_UNSORTED (-6)  /* records not grouped by read (read ids must not decrease)  */
#define KARMA_ERR_STATE (-7)     /* call out of order (e.g. profile before finalize)          */
#define KARMA_ERR_PARSE (-8)     /* input text outside what the C++ parser reproduces exactly */
#define KARMA_ERR_COMM (-9)      /* RCCL communicator error                                   */
#define KARMA_ERR_STALL (-10)    /* a deferred step's status did not arrive (stalled peer/device) */

#define KARMA_KMER_5P6 (-1) /* kmer.py:69 "5p6": all 5-mers + string-palindromic 6-mers */

int karma_version(void);
const char* karma_last_error(void);
/* Build identity as a JSON object: {"arch", "defines" (extra -D flags of a
 * variant build; "" for the shipped library), "src_sha256_16", "flags"}.
 * bench.py prints it and refuses a non-default build. */
const char* karma_build_info(void);
int karma_device_count(int* n);
/* Layout of a context's mapped host region (diagnostic; no device needed):
 * one fixed slot per user, offsets[s] / bytes[s] for s < min(cap, *n). */
int karma_mapped_slots(int64_t* offsets, int64_t* bytes, int cap, int* n);
/* HIP runtime (and RCCL) calls this thread has made through the library that
 * enqueue work, wait, or manage streams, events and memory (launches, copies,
 * memsets, event records, stream waits, synchronisations, collectives). */
int karma_api_calls(uint64_t* n);

/* ---- context: one device, one HIP stream --------------------------------- */
typedef struct karma_ctx karma_ctx;
int karma_ctx_create(int device, karma_ctx** out);
int karma_ctx_destroy(karma_ctx* ctx);
/* Launch on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the context's own stream. */
int karma_ctx_set_stream(karma_ctx* ctx, void* hip_stream);
int karma_ctx_sync(karma_ctx* ctx);
/* Per-kernel HIP-event timing on the launch stream (for bench.py's roofline). */
int karma_timing_enable(karma_ctx* ctx, int on);
/* Restrict timing to launches of one kernel name (NULL or "": every kernel), so a
 * timed region carries two events per launch of that kernel only. */
int karma_timing_only(karma_ctx* ctx, const char* name);
int karma_timing_reset(karma_ctx* ctx);
/* Fills up to cap entries: name (NUL-separated into names[cap*64]), total ms, launches.
 * Returns number of distinct kernels in *n. Synchronises the stream. */
int karma_timing_read(karma_ctx* ctx, char* names, double* total_ms, int64_t* launches, int cap, int* n);

/* ---- device memory helpers (for callers without their own allocator) ------ */
int karma_dev_alloc(karma_ctx* ctx, size_t bytes, void** out);
int karma_dev_free(karma_ctx* ctx, void* p);
int karma_memcpy(karma_ctx* ctx, void* dst, const void* src, size_t bytes, int kind /*0 H2D,1 D2H,2 D2D*/);
/* The same, ordered on the context's stream and not waited for (host memory
 * must stay valid until the stream reaches the copy). */
int karma_memcpy_async(karma_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
/* Pinned host memory for results (device -> host copies into it run at the
 * full PCIe rate): blocks are cached by size class after karma_host_free. */
int karma_host_alloc(size_t bytes, void** out);
int karma_host_free(void* p);
int karma_memset_async(karma_ctx* ctx, void* dst, int value, size_t bytes);
/* Average ms of `reps` hipMemsetAsync of `bytes` at dst (HIP events on the
 * context's stream): the device's write ceiling for a buffer of that size. */
int karma_memset_timed(karma_ctx* ctx, void* dst, size_t bytes, int reps, double* ms);
/* Streams owned by the library (a side stream for the profile, a high-priority
 * main stream); priority: 0 normal, < 0 higher (hipStreamCreateWithPriority). */
int karma_stream_create(karma_ctx* ctx, int priority, void** stream);
int karma_stream_destroy(karma_ctx* ctx, void* stream);
int karma_stream_sync(karma_ctx* ctx, void* stream);

/* ---- RCCL communicator (one per device and process) ----
 * The multi-GPU build's two exchange steps (presence MAX-allreduce + exception
 * all-gather for the column table; pair all-to-all-v + totals all-gather for the
 * graph) run on it, enqueued on the bound context's stream.  The 128-byte unique
 * id made by one rank reaches the others through the caller's bootstrap
 * (karma_amd/hostgroup.py).  Replaces nothing in the reference (single process). */
typedef struct karma_comm karma_comm;
#define KARMA_DT_U8 0
#define KARMA_DT_I32 1
#define KARMA_DT_I64 2
#define KARMA_DT_U64 3
#define KARMA_DT_F64 4
#define KARMA_OP_SUM 0
#define KARMA_OP_MAX 1
#define KARMA_OP_MIN 2
int karma_comm_id_bytes(void);
int karma_comm_unique_id(uint8_t* id);
int karma_comm_create(karma_ctx* ctx, const uint8_t* id, int world, int rank, karma_comm** out);
/* The same with flags.  KARMA_COMM_SIDE: a second communicator over the same
 * ranks (its own unique id) for collectives enqueued on a side stream.  One
 * communicator's operations must be issued in the same order on every rank; a
 * job with collectives on two streams gives each stream its own communicator,
 * so the two orders never interleave differently across ranks. */
#define KARMA_COMM_SIDE 1
int karma_comm_create_ex(karma_ctx* ctx, const uint8_t* id, int world, int rank, int flags, karma_comm** out);
int karma_comm_destroy(karma_comm* c);
int karma_comm_info(karma_comm* c, int* world, int* rank);
/* In place on device memory, stream-ordered. */
int karma_comm_allreduce(karma_comm* c, void* buf_dev, int64_t count, int dtype, int op);
/* Host scalars (at most max(64, 8 * world) bytes); synchronises the stream. */
int karma_comm_allreduce_host(karma_comm* c, void* buf_host, int64_t count, int dtype, int op);
int karma_comm_barrier(karma_comm* c);
/* recv_dev[r * bytes_per_rank ...] = rank r's send_dev; in place when
 * send_dev == recv_dev + rank * bytes_per_rank. */
int karma_comm_allgather(karma_comm* c, const void* send_dev, void* recv_dev, int64_t bytes_per_rank);
/* recv_host[r] = send_host[rank] of rank r (world int64 each; synchronises). */
int karma_comm_exchange_counts(karma_comm* c, const int64_t* send_host, int64_t* recv_host);
/* Bytes send_dev[send_off[r], send_off[r+1]) go to rank r and land in its
 * recv_dev[recv_off[me], ...); offsets are host arrays of world + 1 entries. */
int karma_comm_alltoallv(karma_comm* c, const void* send_dev, const int64_t* send_off, void* recv_dev,
                         const int64_t* recv_off);
/* The same for a list held as two arrays of equal element size (keys and
 * counts): part a and part b of each slice go as two grouped sends, so the
 * sender needs no interleaved copy.  Offsets (bytes) apply to both parts. */
int karma_comm_alltoallv_kv(karma_comm* c, const void* send_a, const void* send_b, const int64_t* send_off,
                            void* recv_a, void* recv_b, const int64_t* recv_off);

/* ---- contig store (device-resident, 2-bit packed + exception mask) -------- */
typedef struct karma_contigs karma_contigs;
/* seq: concatenated sequence bytes (latin-1 code points of the reference's str
 * values), offsets[n+1] into seq, key_len[n] = len(FASTA dict key) — the
 * reference's normaliser (kmer.py:213 iterates the dict's keys).
 * is_device = 0: host pointers, copied; 1: device pointers, referenced (must
 * outlive the store).  Packs A,C,G,T to 2 bits on the device; any other byte is
 * an exception base handled through a byte-key path. */
int karma_contigs_create(karma_ctx* ctx, const uint8_t* seq, const int64_t* offsets, const int32_t* key_len,
                         int64_t n, int is_device, karma_contigs** out);
int karma_contigs_destroy(karma_contigs* c);
int karma_contigs_info(karma_contigs* c, int64_t* n, int64_t* total_bases, int64_t* exception_bases,
                       int64_t* packed_bytes);
/* For tests: the store's arrays copied to the host (a null pointer skips one).
 * packed and mask: one entry per 16 bases, every contig starting on a word
 * (ceil(len / 16) words each, woff[n] in all); packed has the first base in
 * bits 31:30, A C G T = 0 1 2 3 and every other or missing base 0; mask has
 * bit 15 - j set when base j is none of A, C, G, T.  woff: n + 1 word offsets.
 * has_exc: n flags, contig has such a base.  Synchronises the stream. */
int karma_contigs_words(karma_contigs* c, uint32_t* packed, uint16_t* mask, int64_t* woff, uint8_t* has_exc);

/* ---- k-mer profile (kmer.py:146-264) -------------------------------------- */
typedef struct karma_kmer_plan karma_kmer_plan;
/* Presence pass over the (local) contig store. kmode: 1..8 or KARMA_KMER_5P6. */
int karma_kmer_plan_create(karma_ctx* ctx, karma_contigs* c, int kmode, karma_kmer_plan** out);
int karma_kmer_plan_destroy(karma_kmer_plan* p);
/* Multi-rank exchange points: the ACGT presence bitmap (OR /
 * max-reduce across ranks) and the non-ACGT ("exception") k-mer keys (union). */
int karma_kmer_presence_words(karma_kmer_plan* p, int64_t* nwords);
int karma_kmer_presence_get(karma_kmer_plan* p, uint32_t* dst_dev);
int karma_kmer_presence_set(karma_kmer_plan* p, const uint32_t* src_dev);
/* presence = OR of n_sets bitmaps of presence_words each, back to back in
 * device memory (the ranks' bitmaps after an all-gather). */
int karma_kmer_presence_merge(karma_kmer_plan* p, const uint32_t* all_dev, int n_sets);
int karma_kmer_exceptions_count(karma_kmer_plan* p, int64_t* n);
int karma_kmer_exceptions_get(karma_kmer_plan* p, uint64_t* dst_dev);
int karma_kmer_exceptions_set(karma_kmer_plan* p, const uint64_t* src_dev, int64_t n);
/* Column table = sorted() union of present k-mers (kmer.py:172-177). */
int karma_kmer_plan_finalize(karma_kmer_plan* p, int64_t* M);
/* The same in two halves: _async enqueues the column table and M's readback;
 * _wait waits for those alone (not for later work on the stream).  One
 * finalize in flight per context. */
int karma_kmer_plan_finalize_async(karma_kmer_plan* p);
int karma_kmer_plan_finalize_wait(karma_kmer_plan* p, int64_t* M);
/* Column keys: byte-packed u64, big-endian bytes from bit 63; for k < 8 and 5p6
 * the low byte holds the k-mer length (so u64 order == Python str order). */
int karma_kmer_columns(karma_kmer_plan* p, uint64_t* keys_host);
/* Dense float64 profile, row r = contig r of the store, stride ld >= M:
 * out[r*ld + col] = count / key_len[r] (kmer.py:120, :231-233), zeros written. */
int karma_kmer_profile(karma_kmer_plan* p, double* out, int64_t ld, int out_is_device);
/* Rows [row_lo, row_hi) of the same profile: row r of out is contig row_lo + r
 * (SURVEY.md §8(e) streaming: a profile larger than host or device memory is
 * produced and copied out one row block at a time; host output synchronises). */
int karma_kmer_profile_rows(karma_kmer_plan* p, int64_t row_lo, int64_t row_hi, double* out, int64_t ld,
                            int out_is_device);
/* karma_kmer_profile into device memory, launched on `side` (a hipStream_t)
 * after everything already enqueued on the context's stream -- or, while a
 * karma_graph_records_begin job is open, after that job's classify kernel and
 * this plan's column table -- so it overlaps the rest of the stream's work.  Call karma_ctx_join
 * before the plan or the output are used or destroyed.  side = NULL: the
 * context's stream. */
int karma_kmer_profile_side(karma_kmer_plan* plan, double* out_dev, int64_t ld, void* side);
/* The context's stream waits (on the device) for the work enqueued on `side`. */
int karma_ctx_join(karma_ctx* ctx, void* side);
/* Block slots per CU the side-stream profile's grid leaves free for the main
 * stream (default 0: the profile's 3 blocks per CU take the chip; a free slot
 * measured slower). */
int karma_ctx_set_side_headroom(karma_ctx* ctx, int blocks_per_cu);
/* Number of k-mer occurrences per contig (0 => the all-zero row of kmer.py:250-258). */
int karma_kmer_row_totals(karma_kmer_plan* p, int64_t* dst_host);
/* For tests: the sizes the k-mer kernels are laid out by, the first n of:
 * positions and packed words of a stage, zero words behind the store, contigs
 * of the presence pass's first launch, waves per presence block and per
 * profile block, the most columns and the largest ordinal space of the
 * wave-per-contig profile, the most columns of a block's LDS histogram, the
 * size of a row's quotient table, the contig length from which counters are
 * u32, the column table's block size, the most blocks of the pack and of a
 * presence launch.  No device call. */
int karma_kmer_tile(int* v, int n);
/* For tests: the kernel karma_kmer_profile launches for this plan: 0 one wave
 * per contig with u16 counters, 1 the same with u32 counters, 2 one block per
 * contig with its counts in LDS, 3 the same with a scratch row.  use_cap = 0:
 * chosen on M (after finalize); 1: on the most columns the plan can have, as a
 * step that leaves M on the device does.  No device call. */
int karma_kmer_profile_path(karma_kmer_plan* p, int use_cap, int* path);

/* ---- exact k nearest neighbours of matrix rows (the profile's kNN graph) ---- */
/* x: row-major f64, n rows, m columns, row stride ld >= m (in doubles), on the
 * host (x_is_device = 0: copied up) or the device.  For every query row i in
 * [row_lo, row_hi) writes its k nearest rows among all n, itself included:
 *
 *   distance  d2(i, j) is accumulated over the columns c = 0 ... m - 1 in that
 *             order from +0.0: t = x[i,c] - x[j,c]; acc = acc + t * t, each of
 *             the three a single IEEE round-to-nearest f64 operation, no
 *             contraction, subnormals kept: what numpy computes elementwise.
 *             d2(i, j) and d2(j, i) are bit-identical.
 *   order     the k rows j in [0, n) with the smallest (d2(i, j), j),
 *             lexicographically, ascending.  d2 >= +0, so the u64 bit patterns
 *             order the same way.  Row i is not special: it usually comes
 *             first, but a duplicate row with a lower index precedes it.
 *   outputs   idx: int32 (row_hi - row_lo) x k row-major; dist: f64 of the same
 *             shape, the correctly rounded sqrt(d2).  The order is by d2, not
 *             by the rounded root.  Host or device (out_is_device).
 *   limits    1 <= k <= min(n, k_max) (karma_knn_tile; 64); n < 2^31.  n == 0
 *             or row_lo == row_hi: nothing is written, KARMA_OK (pointers and k
 *             are then not looked at).
 *
 * Non-finite inputs (NaN, +-inf) are outside the contract: the k-mer profile
 * never holds them.  d2 = +inf that overflows from finite inputs is inside it
 * and ties by index like any other value.  Padding beyond column m of a row is
 * never read.
 * KARMA_ERR_ARG with a message: a null pointer, k out of range, ld < m, a row
 * range not within 0 <= row_lo <= row_hi <= n, x or dist off an 8-byte boundary
 * (idx: 4-byte), a byte size that overflows.  KARMA_ERR_OOM: no memory for the
 * copy of a host x or for host outputs' device twins.  Synchronises the stream
 * once before returning.  Kernel name in the timing table: profile_knn. */
int karma_knn_rows(karma_ctx* ctx, const double* x, int64_t n, int64_t m, int64_t ld, int x_is_device,
                   int64_t row_lo, int64_t row_hi, int k, int32_t* idx, double* dist, int out_is_device);
/* The kernel's tile, for tests that place cases on its edges: query rows per
 * block, candidate rows per step, columns staged at a time, the largest k. */
int karma_knn_tile(int* query_rows, int* cand_rows, int* col_panel, int* k_max);

/* ---- the same neighbour lists, one block of candidate rows at a time -------- */
/* For profiles that are not one resident matrix (a sharded build's ranks, a
 * streamed profile): per-query lists that outlive a call, folded with one
 * block of candidate rows after another.  Distance, order and tie rule are
 * karma_knn_rows' above; the result of folding every row once, in any block
 * order, then karma_knn_finish, is bit for bit karma_knn_rows' of the whole
 * matrix.
 *
 *   state     keys: u64 nq x k row-major, the d2 bit patterns; idx: int32 of
 *             the same shape.  A row's entries are sorted ascending by
 *             (key, index); an empty slot is (all-ones, INT32_MAX) and sorts
 *             last.  Host or device (state_is_device; both arrays alike).
 *   block     q: nq query rows, c: nc candidate rows, both row-major f64 of m
 *             columns with row strides ldq, ldc >= m, each on the host (copied
 *             up) or the device.  Candidate row r has index cand_base + r.  A
 *             query row that is also among the candidates competes like any
 *             other row.
 *   result    each row's list becomes the k smallest (d2 bits, index) of
 *             {its carried entries} and {this block's candidates}: an equal d2
 *             with a lower index displaces a carried entry, so the order in
 *             which blocks arrive does not matter.  first != 0: the incoming
 *             state is not read (the lists start empty).  nc == 0: the state
 *             stays as it is, or with first becomes all-empty lists.  nq == 0:
 *             nothing is done.  m == 0: every d2 is +0.
 *   split     cand_split = S >= 1: S slices of the block's candidate tiles
 *             (contiguous, whole tiles of karma_knn_tile's cand_rows) run side
 *             by side into partial lists in scratch memory, which a second
 *             kernel merges with the carried list; S is clamped to the number
 *             of tiles and to 32.  The lists do not depend on S.  0: the
 *             library chooses (karma_knn_block_split tells what).
 *   limits    1 <= k <= 64; k may exceed nc.  0 <= cand_base and
 *             cand_base + nc <= 2^31 - 1.  nq < 2^31.  Inputs finite, as above.
 *
 * The caller's contract: across the calls (and merges) that feed one state no
 * candidate index is offered twice; otherwise the lists are unspecified (no
 * error, no fault).
 * KARMA_ERR_ARG with a message, before anything is touched: negative shapes,
 * ldq or ldc < m, cand_base out of range, k out of range, a negative
 * cand_split, a null pointer, a matrix or keys off an 8-byte boundary (idx:
 * 4-byte), a byte size that overflows.  Synchronises the stream once before
 * returning.  Kernel names in the timing table: profile_knn_block, and with
 * S > 1 one profile_knn_merge. */
int karma_knn_block(karma_ctx* ctx, const double* q, int64_t nq, int64_t ldq, int q_is_device,
                    const double* c, int64_t nc, int64_t ldc, int c_is_device,
                    int64_t m, int64_t cand_base, int k,
                    uint64_t* keys, int32_t* idx, int state_is_device,
                    int first, int cand_split);
/* keys / idx (in, out) become, per row, the k smallest (key, index) of
 * themselves and a second list of the same shape and location (keys_b, idx_b:
 * read only).  Both sorted as above; the two must not share a candidate index.
 * Kernel name: profile_knn_merge (one wave per row, no atomics). */
int karma_knn_merge(karma_ctx* ctx, uint64_t* keys, int32_t* idx,
                    const uint64_t* keys_b, const int32_t* idx_b,
                    int64_t nq, int k, int state_is_device);
/* out_idx = idx and out_dist = the correctly rounded sqrt of the d2 whose bits
 * a key holds (nq x k each, host or device); an empty slot comes out as
 * (-1, +inf).  The state is not changed.  Kernel name: profile_knn_finish. */
int karma_knn_finish(karma_ctx* ctx, const uint64_t* keys, const int32_t* idx, int64_t nq, int k, int state_is_device,
                     int32_t* out_idx, double* out_dist, int out_is_device);
/* The split a karma_knn_block call of nq query rows and nc candidate rows runs
 * with for this cand_split: the clamped value, or for 0 the library's choice:
 * the largest S <= 32 with ceil(nq / query_rows) * S blocks within what the
 * device holds at once (compute units x resident blocks of the kernel with
 * the smallest lists), clamped to the tiles.  ctx is needed for 0 only. */
int karma_knn_block_split(karma_ctx* ctx, int64_t nq, int64_t nc, int cand_split, int* used);

/* ---- HDBSCAN: mutual-reachability spanning tree and cluster tree ------------- */
/* x: row-major f64, n rows, m columns, row stride ld >= m (in doubles), on the
 * host (x_is_device = 0: copied up) or the device.  Writes the exact minimum
 * spanning tree of the complete mutual-reachability graph of the rows:
 *
 *   d2(i, j)   karma_knn_rows' definition exactly: the columns in order from
 *              +0.0, t = x[i,c] - x[j,c]; acc = acc + t * t, no contraction.
 *              Symmetric bit for bit.
 *   core2(i)   the min_samples-th smallest (d2(i, j), j) over all j in [0, n),
 *              row i itself counted: the last key of karma_knn_rows with
 *              k = min_samples (scikit-learn's kneighbors(X, min_samples)[:, -1]).
 *              core[i] is the correctly rounded sqrt(core2(i)).
 *   mr2(i, j)  max(d2(i, j), core2(i), core2(j)).  All values are >= +0, so
 *              the u64 bit patterns order them.
 *   tree       the one minimum spanning tree of the complete graph under the
 *              strict total order of the edge keys (mr2(i, j), lo, hi), lo =
 *              min(i, j) < hi.  It does not depend on the algorithm: Kruskal
 *              over all pairs sorted by that key gives these n - 1 edges, and
 *              so does Prim with that comparison.
 *   outputs    the n - 1 edges ascending by that key: a = lo, b = hi (int32),
 *              w = the correctly rounded sqrt(mr2) (f64); core: f64[n].  The
 *              order is by mr2, not by the rounded root.  Host or device
 *              (out_is_device; all four alike).
 *   limits     1 <= min_samples <= min(n, 64); 1 <= n < 2^31; m >= 0, where
 *              m == 0 makes every d2 +0.  n == 1 writes core[0] = 0 and no
 *              edge (a, b and w are then not looked at).
 *
 * Finite inputs only; a d2 that overflows to +inf from finite inputs is inside
 * the contract and ties by index.  min_samples = 1 gives core 0: the plain
 * Euclidean tree.
 * KARMA_ERR_ARG with a message, before a device is looked for: a null pointer,
 * min_samples out of range, ld < m, x, w or core off an 8-byte boundary (a, b:
 * 4-byte), a byte size that overflows.  Boruvka rounds on karma_knn_rows' tile;
 * the host reads one edge count per round and sorts the edges at the end.
 * Kernel names in the timing table: profile_knn_block (the neighbour lists
 * core2 is taken from), mst_core, and per round mst_nearest, mst_reduce (two
 * passes), mst_hook (hook, pointer jumps, relabel). */
int karma_mreach_mst(karma_ctx* ctx, const double* x, int64_t n, int64_t m, int64_t ld, int x_is_device,
                     int min_samples, int32_t* a, int32_t* b, double* w, double* core, int out_is_device);
/* The tile, for tests that place cases on its edges: query rows per block,
 * candidate rows per step, columns staged at a time, and the most rounds any
 * n takes (a round at least halves the components: ceil(log2 n)). */
int karma_mst_tile(int* query_rows, int* cand_rows, int* col_panel, int* rounds_max);
/* From a spanning tree's edges to HDBSCAN labels, on the host (no device, no
 * context).  a, b, w: n - 1 edges in the order given, which must have
 * non-decreasing w (karma_mreach_mst's output order); the order among equal
 * weights is part of the input: it decides left and right below.
 *
 *   linkage    a union-find walks the edges in order; merge e makes node n + e
 *              with left = find(a[e]), right = find(b[e]).
 *   condensing breadth-first from the root, left before right, with lambda =
 *              1 / w (+inf for w == 0).  A split whose two sides both hold at
 *              least min_cluster_size points makes two new clusters, the left
 *              one numbered first; otherwise the large side keeps its parent's
 *              label and the points of a small side fall out at that lambda.
 *   stability  of a label: sum of (lambda - lambda at the label's birth) * size
 *              over what leaves it, in the order the condensing made it.
 *   selection  excess of mass from the deepest label up: a label whose
 *              children's summed stability is larger gives way to them (and
 *              takes that sum), otherwise it is selected and everything below
 *              it is not.  The root is a candidate only with
 *              allow_single_cluster.
 *   labels     selected clusters are numbered 0.. in ascending label; a point
 *              belongs to the nearest selected label above it; noise is -1.
 *              When the root is the one selected cluster, a point is a member
 *              iff its lambda is >= the largest lambda among the root's
 *              children.
 *   prob       min(lambda_point, max_lambda(cluster)) / max_lambda(cluster);
 *              1 where max_lambda is 0 or not finite; 0 for noise.
 *
 * This is scikit-learn 1.7's make_single_linkage followed by tree_to_labels
 * with its defaults (excess of mass, epsilon 0, no maximum cluster size).
 * n >= 1; n == 1 gives label -1, probability 0, zero clusters.
 * min_cluster_size >= 2.  A cluster whose stability is not finite (zero-weight
 * edges) is outside the contract.  KARMA_ERR_ARG, with nothing written: a null
 * pointer, n or min_cluster_size out of range, a weight that is negative, NaN or
 * below the one before it, an endpoint outside [0, n), an edge joining two
 * points that are joined already. */
int karma_hdbscan_tree(int64_t n, const int32_t* a, const int32_t* b, const double* w,
                       int min_cluster_size, int allow_single_cluster,
                       int32_t* labels, double* prob, int32_t* n_clusters);

/* ---- UMAP: fuzzy neighbour graph and layout ------------------------------------ */
/* The step between the neighbour lists and HDBSCAN.  Every output bit is
 * defined here; equality with umap-learn's coordinates is not claimed (its
 * layout is a racy parallel SGD with its own generator).
 *
 *   kexp(x)   x = min(max(x, -745.0), 709.0); n = rint(x * LOG2E);
 *             r = (x - n * LN2_HI) - n * LN2_LO; p = 1/13!; then for d = 12!,
 *             11!, ..., 1!, 0!: p = p * r + 1.0 / d (the correctly rounded
 *             quotients); h = floor(n * 0.5);
 *             kexp = ldexp(ldexp(p, (int)h), (int)(n - h)).
 *   klog(x)   x > 0 finite: (m, e) = frexp(x); if m < 0.7071067811865476:
 *             m = m * 2.0, e = e - 1; f = m - 1.0; s = f / (2.0 + f); z = s * s;
 *             p = 1/23; then for d = 21, 19, ..., 3, 1: p = p * z + 1.0 / d;
 *             klog = e * LN2_HI + ((2.0 * s) * p + e * LN2_LO).
 *   kpow(x, b) = kexp(b * klog(x)), x > 0.
 *   LOG2E = 1.4426950408889634, LN2_HI = 6.93147180369123816490e-01,
 *   LN2_LO = 1.90821492927058770002e-10.  Every step is one IEEE f64 + - * /,
 *   a comparison, rint, floor, frexp or ldexp; no contraction (csrc/umap_math.h).
 *   kexp is within 2.2e-16 of exp, klog within 4.4e-16 of log (relative).
 *
 * karma_umap_graph: the fuzzy simplicial set of neighbour lists idx (int32) and
 * dist (f64), n x k row-major as karma_knn_rows / karma_knn_finish write them,
 * on the host (in_is_device = 0: copied up) or the device.
 *
 *   rho(i)    the first dist[i, j] > 0 in list order, 0 if there is none
 *             (umap's local_connectivity = 1).
 *   sigma(i)  umap's smooth_knn_dist bisection with target = log2((double)k):
 *             lo = 0, hi = +inf, mid = 1; at most 64 times: psum from +0.0 over
 *             the entries j = 0 .. k - 1 in order with idx[i, j] != i, with
 *             d = dist[i, j] - rho(i): psum = psum + (d > 0 ? kexp(-(d / mid))
 *             : 1.0); stop if |psum - target| < 1e-5; else if psum > target:
 *             hi = mid, mid = (lo + hi) / 2.0; else lo = mid, mid = mid * 2.0
 *             while hi is +inf, otherwise (lo + hi) / 2.0.  Then sigma(i) =
 *             max(mid, 1e-3 * mean): the row's in-order sum of its k distances
 *             / k where rho(i) > 0, otherwise the global mean: the row sums
 *             added in row order from +0.0, / (double)(n * k).
 *   A[i, c]   for an entry with c = idx[i, j] != i and d = dist - rho(i): 1.0
 *             if d <= 0 or sigma(i) == 0, otherwise kexp(-(d / sigma(i))).
 *             Entries naming the row itself are dropped.
 *   w(i, c)   with p = A[i, c], q = A[c, i], each 0 where absent:
 *             (p + q) - p * q (umap's set_op_mix_ratio = 1): bit-symmetric.
 *             Entries with w == 0 are dropped.
 *   outputs   CSR: indptr int64[n + 1]; indices int32[nnz], each row ascending
 *             by column; weights f64[nnz]; *nnz (always a host word).  The
 *             result is a sorted set: it does not depend on the algorithm.
 *             indices and weights hold cap >= 2 n k entries (the bound of nnz).
 *             sigma, rho: f64[n], optional (null: not written).  Outputs on the
 *             host or the device (out_is_device; all alike).
 *   limits    2 <= k <= min(n, 64); 2 <= n < 2^31; 2 n k < 2^32.  A list must
 *             not name a row twice (karma_knn_rows' never do).
 *
 * KARMA_ERR_ARG with a message, before a device is looked for: a null pointer,
 * n or k out of range, cap < 2 n k, misalignment (f64 / int64: 8 bytes, int32:
 * 4), a byte size that overflows, a host list naming a row outside [0, n).  A
 * device list naming such a row is found by the first kernel: KARMA_ERR_ARG,
 * nothing indexed with it.  Kernel name in the timing table: umap_graph (rows,
 * sigma, entries, indptr, gather) around one radix sort of 2 n k keys. */
int karma_umap_graph(karma_ctx* ctx, const int32_t* idx, const double* dist, int64_t n, int k, int in_is_device,
                     int64_t* indptr, int32_t* indices, double* weights, int64_t cap, int64_t* nnz,
                     double* sigma, double* rho, int out_is_device);
/* Rows (vertices) per block of the graph's and the layout's per-row kernels,
 * for tests that place cases on block edges. */
int karma_umap_tile(int* rows_per_block);
/* karma_umap_layout: the layout of a symmetric CSR graph (karma_umap_graph's
 * output; host or device, graph_is_device) in gather form.  y: f64 n x dim
 * row-major, in and out, host or device (y_is_device).
 *
 *   start     init != 0: y is first filled with y[i, c] = -10.0 + 20.0 *
 *             ((splitmix64(seed + (i * dim + c + 1) * 0x9E3779B97F4A7C15) >> 11)
 *             * 2^-53) (umap's init="random"); splitmix64(z): z = (z ^ z >> 30)
 *             * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *             z ^ z >> 31 (u64).  init == 0: the caller's y.
 *   schedule  per directed CSR entry e (row i, column j, weight w), wmax the
 *             largest weight: active iff w >= wmax / (double)n_epochs (umap's
 *             pruning; an inactive entry never fires but keeps its number e);
 *             eps = wmax / w; eons = eps; epns = eps / (double)R; eonns = epns;
 *             a u32 counter t_e = 0.  R = negative_sample_rate; R == 0: no
 *             negatives.
 *   epoch     ep = 0 .. n_epochs - 1, alpha = initial_alpha * (1.0 -
 *             (double)ep / (double)n_epochs).  For every vertex i independently:
 *             cur = Y_old[i]; for each active entry of row i in CSR order with
 *             eons <= (double)ep:
 *               attract  o = Y_old[j]; df[c] = cur[c] - o[c]; d2 = the in-order
 *                        sum from +0.0 of df[c] * df[c]; if d2 > 0: pb =
 *                        kpow(d2, b); g = ((-2.0 * a * b) * (pb / d2)) / (a * pb
 *                        + 1.0); cur[c] = cur[c] + clip4(g * df[c]) * alpha,
 *                        clip4 clamping to [-4, 4].
 *               eons = eons + eps; nneg = (int)(((double)ep - eonns) / epns).
 *               repel    nneg times: kk = splitmix64((seed ^ (e *
 *                        0xD1342543DE82EF95)) + (t_e + 1) * 0x9E3779B97F4A7C15)
 *                        mod n (u64); t_e += 1; o = Y_old[kk]; df, d2 as above;
 *                        if d2 > 0: g = (2.0 * gamma * b) / ((0.001 + d2) * (a *
 *                        kpow(d2, b) + 1.0)) and the same update; d2 == 0 (kk ==
 *                        i among others): no move.
 *               eonns = eonns + (double)nneg * epns.
 *             Y_new[i] = cur.  Then the buffers swap.
 *
 * A vertex moves only through its own row; the graph is symmetric, so the entry
 * (j, i) moves j by its own schedule (umap's move_other).  Own coordinates are
 * live, everyone else's are those of the epoch's start: no race, no float
 * atomic, and the result does not depend on block shape or launch order.
 * limits: 1 <= dim <= 16; n_epochs >= 1; R >= 0; 2 <= n < 2^31; a, b, gamma,
 * initial_alpha finite; weights finite and > 0.
 * KARMA_ERR_ARG with a message: a null pointer, a range above, misalignment, a
 * byte size that overflows, indptr not starting at 0, decreasing or not ending
 * at nnz, a column outside [0, n), a bad weight -- for a host graph before a
 * device is looked for, for a device graph by the first kernel, before anything
 * is indexed with it.  One launch per epoch and no host wait between them; a
 * hub's row is walked by the one thread that owns it.  Kernel name in the
 * timing table: umap_layout. */
int karma_umap_layout(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights,
                      int64_t n, int64_t nnz, int graph_is_device, int dim, double a, double b, int n_epochs,
                      int negative_sample_rate, double gamma, double initial_alpha, uint64_t seed, int init,
                      double* y, int y_is_device);
/* umap's find_ab_params on the host (no device, no context): the least-squares
 * fit of 1 / (1 + a x^(2b)) on the 300 points of linspace(0, 3 spread, 300) to
 * 1 for x < min_dist, else exp(-(x - min_dist) / spread), by Levenberg-Marquardt
 * from a = b = 1.  Agrees with scipy's curve_fit to its tolerances; a and b are
 * inputs of the layout, whose bit contract does not rest on this fit.
 * KARMA_ERR_ARG: a null pointer, spread not finite and > 0, min_dist not finite
 * and >= 0. */
int karma_umap_ab(double spread, double min_dist, double* a, double* b);

/* ---- UMAP: spectral start, component by component ------------------------------ */
/* karma_graph_components: the connected components of a CSR graph read as
 * undirected (an entry (i, j) joins i and j; weights are not looked at).
 * comp[i] (int32[n], host or device: comp_is_device) is the smallest vertex of
 * i's component; *n_comp (host) their number.  Labels hook to the minimum and
 * jump to the root in rounds, the host reading one "changed" word per round; at
 * most 2 ceil(log2 n) + 1 rounds (spectral_args.h argues the bound), beyond
 * which KARMA_ERR_STATE.  Integer atomics only: the result is a set property.
 * 1 <= n < 2^31.  KARMA_ERR_ARG as karma_umap_layout's (a host graph before a
 * device is looked for, a device graph by the first kernel).  Kernel name in the
 * timing table: graph_components. */
int karma_graph_components(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz,
                           int graph_is_device, int32_t* comp, int comp_is_device, int64_t* n_comp);
/* karma_spectral_apply: out = S x for a block x (f64 n x p row-major, 1 <= p <=
 * 32; x and out both host or both device: x_is_device), S = D^-1/2 W D^-1/2 of
 * the CSR graph, every bit defined:
 *   d(i)    the in-order sum from +0.0 of row i's weights; isd(i) = 1.0 /
 *           sqrt(d(i))
 *   (S x)[i, c] = isd(i) * (the sum over row i's entries (column j, weight w)
 *           in CSR order, from +0.0, of (w * isd(j)) * x[j, c]); +0.0 for an
 *           empty row, which is a component of its own
 * each step one IEEE f64 operation, no contraction.  A row's loads do not depend
 * on its running sum: only the additions chain. */
int karma_spectral_apply(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights,
                         int64_t n, int64_t nnz, int graph_is_device, const double* x, int p, double* out,
                         int x_is_device);
/* Rows per tile of the solver's reordered block, the block's guard columns
 * (p = dim + guard) and the Chebyshev filter's degree, for tests and tools. */
int karma_spectral_tile(int* rows_per_tile, int* guard, int* degree);
/* Wall milliseconds of this thread's last karma_umap_spectral, for tools: ms[0]
 * labelling the components, ms[1] the reorder, ms[2] the outer rounds, ms[3]
 * (inside ms[2]) the host's small dense problems. */
int karma_spectral_last_ms(double* ms);
/* The solver's small symmetric eigenproblem on the host (no device, no
 * context): cyclic Jacobi on the p x p matrix (a + a^T) / 2, 1 <= p <= 33;
 * w[p] the eigenvalues descending, column k of v (v[i * p + k]) the k-th
 * eigenvector.  KARMA_ERR_STATE if 64 sweeps do not settle it. */
int karma_spectral_jacobi(const double* a, int p, double* w, double* v);
/* karma_umap_spectral: start coordinates y (f64 n x dim) for karma_umap_layout
 * (init == 0) from the bottom eigenvectors of the normalised Laplacian of a
 * symmetric CSR graph (karma_umap_graph's), solved per connected component.
 * This is umap's per-component spectral layout (multi_component_layout) with
 * its meta-placement of the components restated without the data matrix;
 * equality with umap-learn's coordinates is not claimed.  Optional outputs
 * (null: not written): vec, lam, res (f64 n x dim each), comp (int32[n]); all
 * outputs host or device (out_is_device); info (int64[4], host): components,
 * components not converged, outer rounds run, operator applications.
 *
 * Exact, bit for bit:
 *   operator    karma_spectral_apply's S; components karma_graph_components'.
 *   per component C (s vertices, smallest vertex r, m = min(dim, s - 1)):
 *     vec[i, c] (i in C, c < m) is the unit eigenvector of S restricted to C for
 *     its c-th largest eigenvalue theta_c on the complement of sqrt(d), its
 *     sign fixed so that the entry of largest magnitude, first by vertex, is
 *     positive; columns c >= m are +0.0.  lam[r, c] = 1 - theta_c, res[r, c] =
 *     |S v - theta_c v|_2 as the solver measured it; rows of other vertices
 *     hold +0.0.  C is converged iff its m residuals are all <= tol (a single
 *     vertex always is).
 *   composition unit(sd, i, c) = (splitmix64(sd + (i * dim + c + 1) *
 *     0x9E3779B97F4A7C15) >> 11) * 2^-53 (karma_umap_layout's start, u64
 *     arithmetic);
 *       centre_C[c] = (-10.0 + 20.0 * unit(seed, r, c)) * (1.0 - (double)s /
 *                     (double)n)         (one connected graph is centred at 0)
 *       R_C    = 10.0 * kpow((double)s / (double)n, 1.0 / (double)dim)
 *       vmax_C = the largest |vec[i, c]| over i in C, c < m
 *       y[i, c] = (centre_C[c] + (R_C / vmax_C) * vec[i, c]) + 1e-4 * (-1.0 +
 *                 2.0 * unit(seed + 1, i, c)); for m == 0 or c >= m:
 *                 centre_C[c] + 1e-4 * (...).  The last term plays the part of
 *                 umap's noise: coincident points would never part (d2 == 0
 *                 makes no move).
 *     A component that did not converge takes karma_umap_layout's random start
 *     on its rows: y[i, c] = -10.0 + 20.0 * unit(seed, i, c).
 * Judged by properties, not bits (as karma_umap_ab's fit): the eigenvectors
 * themselves.  The solver is a Chebyshev-filtered subspace iteration with
 * Rayleigh-Ritz on a block of dim + 6 columns, at most max_outer rounds per
 * component; it is deterministic -- no float atomics, every reduction in an
 * order fixed by the graph's shape -- so two calls, and a host and a device
 * graph, give the same bytes.  A component that does not converge is reported
 * in res and info, not as an error.
 * limits: 1 <= dim <= 16; 2 <= n < 2^31; tol finite and > 0; max_outer >= 1;
 * weights finite and > 0; the graph symmetric (not checked: an asymmetric one
 * does not converge).  KARMA_ERR_ARG as karma_umap_layout's.  Kernel name in the
 * timing table: umap_spectral. */
int karma_umap_spectral(karma_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* weights,
                        int64_t n, int64_t nnz, int graph_is_device, int dim, uint64_t seed, double tol, int max_outer,
                        double* y, double* vec, double* lam, double* res, int32_t* comp, int out_is_device,
                        int64_t* info);

/* ---- shared-read graph ----------------------------------------------------- */
/* A pair list: unique keys (a << 32 | b, a <= b) sorted ascending with int64
 * counts (and, for eq classes, the first emission position). */
typedef struct karma_pairs karma_pairs;
#define KARMA_REC_SORTED 0   /* records grouped by read, read ids non-decreasing (SAM order) */
#define KARMA_REC_UNSORTED 1 /* any order: sorted by read on the device first, then run as KARMA_REC_FLAGGED words */
#define KARMA_REC_FLAGGED 2  /* records as n_records x u32: contig | (first record of its read) << 31, grouped by
                              * read.  The graph depends only on which records share a read (read_graph.py:31-49
                              * intersects readsets), so the read ids give way to read-start flags: 4 bytes per
                              * record instead of 8.  Record 0 always starts a read; contig ids < 2^31.
                              * The words no longer carry read ids, so the format itself cannot be checked for
                              * grouping (records of ids A, B, A are three reads here, where KARMA_REC_SORTED
                              * reports KARMA_ERR_UNSORTED): whoever makes the words checks it, as
                              * karma_records_flag does on the device (KARMA_ERR_UNSORTED when read ids
                              * decrease) and karma_amd.engine.flag_records on the host (ValueError). */
/* records: n_records x {u32 read_id, u32 contig} interleaved (or, flags =
 * KARMA_REC_FLAGGED, n_records x u32 flagged contigs; records is then a
 * uint32_t array of n_records entries).  Deduplicates
 * (read, contig) (contig.py:11 keeps QNAMEs in a set); emits for every read's
 * contig set S every pair a <= b of S: the diagonal (a, a) counts |readset(a)|,
 * (a, b) counts |R_a ∩ R_b| (read_graph.py:34). */
int karma_graph_records(karma_ctx* ctx, const uint32_t* records, int64_t n_records, int64_t n_contigs, int flags,
                        int is_device, karma_pairs** out);
/* karma_graph_records in two halves.  _begin enqueues the pipeline up to its
 * one host synchronisation and returns; the caller may enqueue other work (on
 * another stream) before _end waits, checks and assembles the list.  Device
 * records must stay valid until _end.  One open job per context; _end always
 * consumes the job (also on error). */
typedef struct karma_graph_job karma_graph_job;
int karma_graph_records_begin(karma_ctx* ctx, const uint32_t* records, int64_t n_records, int64_t n_contigs,
                              int flags, int is_device, karma_graph_job** job);
int karma_graph_records_end(karma_graph_job* job, karma_pairs** out);
/* Owner bounds (nranks + 1 contig ids) of the exchange that will split the
 * next records job's list on this context: the job finds each owner's start
 * on the device as it builds the list, and karma_pairs_split with the same
 * bounds then answers without a launch or a synchronisation.  Applies to one
 * job; at most 64 ranks. */
int karma_graph_split_hint(karma_ctx* ctx, const int64_t* bounds, int nranks);
/* {u32 read, u32 contig} pairs -> KARMA_REC_FLAGGED words, on the device: the
 * producer of the format for a caller whose pairs are on the host or already
 * in HBM (the words then go to karma_graph_records / karma_step_run).
 * rec_format: KARMA_REC_SORTED (read ids must not decrease: KARMA_ERR_UNSORTED
 * otherwise, the pairs path's own condition and message) or KARMA_REC_UNSORTED
 * (stably sorted by read id on the device first, so the words are a function
 * of the input alone; < 2^31 records, as karma_graph_records).  A contig id
 * >= 2^31 is KARMA_ERR_ARG.  records: n_records pairs, host (is_device = 0) or
 * device, any 4-byte alignment; out: n_records u32, host or device, any 4-byte
 * alignment (pointers off a 16-byte boundary go through an aligned temporary);
 * ranges that overlap are KARMA_ERR_ARG.  n_reads (may be NULL): the number of
 * flag bits set.  Synchronises the stream once; after an error the contents of
 * out are unspecified.  n_records == 0: nothing written, *n_reads = 0.
 * (A karma_graph_records job on KARMA_REC_UNSORTED records takes the same
 * route by itself: sort, flagged words, the flagged classify.) */
int karma_records_flag(karma_ctx* ctx, const uint32_t* records, int64_t n_records, int rec_format, int is_device,
                       uint32_t* out, int out_is_device, int64_t* n_reads);
/* The sorted kernel's tile, for tests that place cases on its edges: records
 * per thread (one 16-byte store), per wave and per block. */
int karma_records_flag_tile(int* per_thread, int* per_wave, int* per_block);
/* For tests: launches of the records job's classify kernel this thread has
 * made, by the record format it read (pairs; flagged words).  A function of
 * the call sequence alone, like karma_api_calls. */
int karma_classify_launches(uint64_t* pairs, uint64_t* flagged);
/* For tests: the resident blocks per compute unit (the occupancy query, with
 * the job's dynamic LDS) of the classify kernel a records job of n_contigs in
 * rec_format (KARMA_REC_SORTED or KARMA_REC_FLAGGED) would launch. */
int karma_graph_classify_occupancy(karma_ctx* ctx, int64_t n_contigs, int rec_format, int* blocks_per_cu);
/* For tests: what the code path of a records job of n_records records over
 * n_contigs contigs (at most 2^21, the compact path) is made of, from the
 * function the job itself sets up with (KARMA_CHUNK, KARMA_BIN and
 * KARMA_PART_RESIDENT in the environment are honoured as a job honours them;
 * rec_format selects no different geometry today).  v[n], n ==
 * KARMA_CODE_GEOMETRY_WORDS:
 *   0 code buckets Bc            1 their width bwc (2^bwc contigs)
 *   2 records per classify chunk 3 chunks (one code list each)
 *   4 path: 0 no compact codes, 1 binned classify, 2 per-flush partition,
 *     3 appended runs            5 chunk lists per partition block
 *   6 partition blocks           7 codes per flush of the path's partition
 *   8 reduce groups per bucket     kernel (0: none runs)
 *   9 that kernel's resident blocks per compute unit (the occupancy query) */
#define KARMA_CODE_GEOMETRY_WORDS 10
int karma_graph_code_geometry(karma_ctx* ctx, int64_t n_contigs, int64_t n_records, int rec_format, int64_t* v,
                              int n);
/* Salmon eq classes (read_graph.py:75-114): cls_off[n_classes+1] into members
 * (contig indices as listed, duplicates kept), counts[n_classes], pair_skip[c]=1
 * when the eq_size token is "1" (read_graph.py:102).  Totals (read_graph.py:86-92)
 * go to the pair list's totals array; pairs carry first-emission positions. */
int karma_graph_eq(karma_ctx* ctx, const int64_t* cls_off, const uint32_t* members, const int64_t* counts,
                   const uint8_t* pair_skip, int64_t n_classes, int64_t n_contigs, int is_device, karma_pairs** out);
/* karma_graph_eq from compact host inputs (10 bytes per class fewer over PCIe):
 * sizes[C] = member count (<= 127) | 0x80 when the class's eq_size token is
 * "1" (pair_skip), counts[C] as u32; n_members = the sizes' sum (KARMA_ERR_ARG
 * when they disagree, checked on the device).  Same pairs, firsts and totals. */
int karma_graph_eq_compact(karma_ctx* ctx, const uint8_t* sizes, const uint32_t* members, int64_t n_members,
                           const uint32_t* counts, int64_t C, int64_t n_contigs, karma_pairs** out);
/* Merge (key, count) lists in any order into one sorted unique list (exchange merge). */
int karma_pairs_merge(karma_ctx* ctx, const uint64_t* keys, const int64_t* counts, int64_t n, int is_device,
                      karma_pairs** out);
/* Merge runs [run_off[r], run_off[r + 1]) of (key, count), each sorted by key
 * (the slices an exchange owner receives, one per sender), into one sorted
 * unique list: a pairwise merge tree, then equal keys summed.
 * KARMA_ERR_UNSORTED when a run is not sorted.  run_off is a host array of
 * n_runs + 1 offsets starting at 0. */
int karma_pairs_merge_runs(karma_ctx* ctx, const uint64_t* keys, const int64_t* counts, const int64_t* run_off,
                           int n_runs, int is_device, karma_pairs** out);
/* The merge kernels' constants, for tests that place cases on their edges:
 * elements of a run per block, window keys a block can stage in LDS, runs
 * merged in one ranking pass, and lanes per window-bound search. */
int karma_merge_tile(int* tile, int* lds_keys, int* max_runs, int* search_group);
/* The same for the deferred step's tail (karma_step_run with KARMA_STEP_DEFER:
 * its merge and edge stage are kernels of their own).  Fills the first n of
 * v[0..7]: merge tile elements, window keys a block can stage in LDS, the most
 * runs whose searches run in lockstep, lanes per window-bound search, edge
 * stage tile elements, the most runs (owners), and the most blocks the merge
 * and the edge stage are launched with on ctx's device (both 0 when ctx is
 * NULL: the constants alone need no device). */
int karma_step_tail_tile(karma_ctx* ctx, int* v, int n);
/* The exchange's wire format: n x {i64 key, i64 count} interleaved in device
 * memory.  _get_kc writes the list in it (stream-ordered, not waited for);
 * _merge_runs_kc merges received runs of it (at most 64 runs: without a host
 * synchronisation, equal keys of different runs left adjacent for the edge
 * stage; accessors of the list sum them first). */
int karma_pairs_get_kc(karma_pairs* p, int64_t* kc_dev);
int karma_pairs_merge_runs_kc(karma_ctx* ctx, const int64_t* kc_dev, const int64_t* run_off, int n_runs,
                              karma_pairs** out);
int karma_pairs_destroy(karma_pairs* p);
/* Later kernels on p run on ctx's stream (after p's current stream is drained);
 * p's memory stays with the allocator that made it.  Lets a list built on a
 * second context (concurrent graph build) join the main stream's exchange. */
int karma_pairs_rebind(karma_pairs* p, karma_ctx* ctx);
int karma_pairs_count(karma_pairs* p, int64_t* n);
/* Device pointers of the list (valid until destroy): keys u64[n], counts i64[n]. */
int karma_pairs_device(karma_pairs* p, const uint64_t** keys, const int64_t** counts);
/* Copy the list out.  Host copies (is_device = 0) have completed on return;
 * device copies (is_device = 1) are ordered on p's stream and not waited for. */
int karma_pairs_get(karma_pairs* p, uint64_t* keys, int64_t* counts, uint64_t* first, int is_device);
/* Index of the first key with a >= bounds[r] for r = 0..nranks (host out; searched on the device). */
int karma_pairs_split(karma_pairs* p, const int64_t* bounds, int nranks, int64_t* starts);
/* karma_pairs_split and karma_pairs_get_kc in one launch (the exchange's send
 * side): starts on the host when it returns, kc_dev (n x {key, count}) written. */
int karma_pairs_split_kc(karma_pairs* p, const int64_t* bounds, int nranks, int64_t* starts, int64_t* kc_dev);
/* totals[c] = count of the diagonal pair (c, c) (readset sizes) for c in [0, n_contigs). */
int karma_pairs_totals(karma_pairs* p, int64_t* totals_dev, int64_t n_contigs);

typedef struct karma_edges karma_edges;
#define KARMA_MODE_READS 0 /* diagonal = readset sizes; off-diagonal = shared reads   */
#define KARMA_MODE_EQ 1    /* totals from the eq pass; diagonal pairs are self-loops */
/* Edges with non-zero shared count and weight (s/tot[a] + s/tot[b]) / 2.
 * totals_dev: int64[n_contigs] device array, or NULL to take it from the pair
 * list (diagonal in READS mode, eq totals in EQ mode).  Contract (here and in
 * karma_edges_begin; not checked): every contig id of the list is < n_contigs,
 * and in READS mode with the totals taken from the list every key has a <= b. */
int karma_edges_from_pairs(karma_ctx* ctx, karma_pairs* p, int mode, const int64_t* totals_dev, int64_t n_contigs,
                           karma_edges** out, int64_t* n_edges);
/* The same in two halves, for an all-gather of the totals in between (the
 * sharded build: each owner's diagonal holds the readset sizes of the contigs
 * it owns).  _begin takes the totals from the list (as totals_dev = NULL
 * above), launches the edge count and returns the device totals array
 * (int64[n_contigs], owned by the edges) for the caller to fill further;
 * _end launches the weights and synchronises.  p must stay valid until _end.
 * A list from karma_pairs_merge_runs_kc may hold equal adjacent keys (not yet
 * summed): the edge stage sums them, and reports KARMA_ERR_UNSORTED for a
 * merge input that was not sorted. */
int karma_edges_begin(karma_ctx* ctx, karma_pairs* p, int mode, int64_t n_contigs, karma_edges** out,
                      int64_t** totals_dev);
int karma_edges_end(karma_edges* e, int64_t* n_edges);
/* n_edges = NULL: _end launches the weights and returns at once; the edge
 * count, and the zero-total and merge-order errors, come with the first
 * karma_edges_count / _get / _totals (one synchronisation there). */
int karma_edges_count(karma_edges* e, int64_t* n_edges);
int karma_edges_destroy(karma_edges* e);
/* Any output pointer may be NULL. first is only meaningful in EQ mode. */
int karma_edges_get(karma_edges* e, uint32_t* a, uint32_t* b, int64_t* shared, double* weight, uint64_t* first,
                    int is_device);
int karma_edges_totals(karma_edges* e, int64_t* totals, int is_device);
/* karma_edges_get and karma_edges_totals with one synchronisation. */
int karma_edges_get_all(karma_edges* e, uint32_t* a, uint32_t* b, int64_t* s, double* w, uint64_t* first,
                        int64_t* totals, int is_device);
/* Eq-class edge stages (KARMA_MODE_EQ) only: a, b, w[E] in the reference's
 * insertion order -- edges grouped by a ascending, inside a group by the pair's
 * first emission (read_graph.py:96-131 adds (u, v) from u as pairs are first
 * seen; cls(incoming_graph_data=) keeps that order, read_graph.py:148).  The
 * order is computed on the device; one synchronisation. */
int karma_edges_get_ordered(karma_edges* e, uint32_t* a, uint32_t* b, double* w, int is_device);

/* ---- one rank's step of the sharded build ---------------
 * The whole hot path of one batch on this rank as one call: the records job
 * (read_graph.py:19-50 via Contig readsets, contig.py:4-35) on a main stream,
 * the k-mer column table and dense profile (kmer.py:146-264) on a side stream,
 * and, with several owners, the owners' split, the key/count all-to-all-v, the
 * owner's merge and the edge stage around the totals all-gather.  Replaces the
 * Python per-step sequence of karma_amd/distributed.py (which stays for the
 * host-staged rehearsal transport).
 * comm: the communicator (NULL or world 1: one process); by default every
 * collective of a step goes to it on ONE stream, in the same order on every rank.
 * side_comm: NULL (or comm) for that default; a distinct KARMA_COMM_SIDE
 * communicator puts the column-set exchange on it, on the side stream.
 * bounds[nranks + 1]: owner contig ranges tiling [0, n_glob); this rank's store
 * holds [bounds[rank], bounds[rank + 1]) (nranks = 1: any shard of the n_glob
 * contig ids, no exchange).  One process with nranks > 1 emulates
 * rank `rank` of an nranks-rank job (the exchange's local work, no collectives).
 * The step owns two streams; inputs stay on the device (records: n x {u32 read,
 * u32 contig}, grouped by read). */
typedef struct karma_step karma_step;
#define KARMA_STEP_KEEP 1       /* outputs kept for karma_step_profile / _columns / _edges */
#define KARMA_STEP_SEQUENTIAL 2 /* every kernel on the main stream (per-kernel timing) */
#define KARMA_STEP_FLAGGED 8    /* records_dev in the KARMA_REC_FLAGGED format (n_records x u32) */
#define KARMA_STEP_DEFER 4      /* outputs not read: the step returns without waiting for anything (its
                                 * checks arrive through mapped memory and are read <= 3 steps later; a
                                 * step needing the general path runs again synchronously; a status later
                                 * than KARMA_STEP_STALL_S seconds (120) is KARMA_ERR_STALL).  A status is
                                 * read only at points the call sequence fixes, never because it has
                                 * already landed: by the third deferred step after its own (which waits
                                 * for it), by the next synchronous step -- one of the 8 deferred calls
                                 * that run synchronously after a re-run included, which checks every
                                 * pending step -- and by karma_step_sync.  The counters of
                                 * karma_step_info therefore follow from the order of calls alone.
                                 * records_dev must be 16-byte aligned (without KARMA_STEP_KEEP; checked
                                 * on entry, before any state changes, whether or not the call ends up
                                 * deferred: KARMA_ERR_ARG); other steps take any 4-byte (flagged) or
                                 * 8-byte aligned pointer and copy when they must.  Several ranks:
                                 * once a synchronous step has sized the
                                 * exchange's slots and the store is ACGT-only on every rank (else the
                                 * step runs synchronously, its edge count not read back); every rank
                                 * learns every rank's re-run verdict from the exchange, so all of them
                                 * re-run the same steps.  Every rank must pass the same flags.
                                 * Inputs must stay valid until the next non-deferred step or
                                 * karma_step_sync. */
int karma_step_create(karma_ctx* ctx, karma_comm* comm, karma_comm* side_comm, int kmode, int64_t n_glob,
                      const int64_t* bounds, int nranks, int rank, karma_step** out);
/* info (may be NULL): [0] M, [1] local edges (-1: not read), [2] local pair list
 * size, [3] its summed counts (the last two with KARMA_STEP_KEEP, else -1). */
int karma_step_run(karma_step* s, karma_contigs* store, const uint32_t* records_dev, int64_t n_records, int flags,
                   int64_t* info);
/* Waits for every enqueued step and checks the deferred ones. */
int karma_step_sync(karma_step* s);
/* [M, E, pairs, entries, synchronous steps, deferred steps, re-run steps, pending, host ns inside
 * karma_step_run, of which ns waiting for a deferred step's status, deferred steps on two main
 * streams, deferred steps whose tail ran on the exchange stream, mode bits (1 one communicator,
 * 2 exchange stream allowed, 4 deferral across ranks allowed), ranks, deferred records jobs on the
 * step's own (pre-zeroed) control block] (first n).  After
 * karma_step_sync, M and E are the newest step's also when it was deferred (E: this rank's
 * edges). */
int karma_step_info(karma_step* s, int64_t* info, int n);
/* Outputs (valid until the next run).  _profile: the newest step's profile
 * (device, rows x M dense f64; a deferred step's once karma_step_sync has read
 * its column count).  _columns and _edges: the last KARMA_STEP_KEEP step's
 * column keys and edges (owned by the step: read with karma_edges_get /
 * _totals, never destroyed). */
int karma_step_profile(karma_step* s, double** dev, int64_t* rows, int64_t* M);
int karma_step_columns(karma_step* s, uint64_t* keys_host);
int karma_step_edges(karma_step* s, karma_edges** e);
/* The newest step's graph as this rank owns it (edges with a in its owner
 * range; one process: all), valid after karma_step_sync until the next run.
 * A deferred step's come from its own tail buffers -- the outputs of the
 * kernels a stream of deferred batches runs (step_edge_count / _write, and with
 * an exchange step_pack / step_merge) -- a synchronous one's (a re-run
 * included) from its karma_edges.  *n_edges = E; *deferred (may be NULL) = 1
 * for a deferred step's.  a, b, shared, weight: E entries each (E <= cap, else
 * KARMA_ERR_ARG), sorted by (a, b), a < b, weight (s/|A| + s/|B|)/2
 * (read_graph.py:19-50, :34-42); totals: n_glob readset sizes.  Any pointer may
 * be NULL (all NULL: only the count). */
int karma_step_newest_edges(karma_step* s, uint32_t* a, uint32_t* b, int64_t* shared, double* weight,
                            int64_t* totals, int64_t cap, int is_device, int64_t* n_edges, int* deferred);
int karma_step_destroy(karma_step* s);

/* ---- synthetic inputs (spec in karma_amd/synth.py) ------- */
int karma_synth_contig_lengths(uint64_t seed, int64_t n, int32_t len_min, int32_t len_span, int64_t* lengths);
/* Fills seq[total] given offsets[n+1] (prefix sums of the lengths). */
int karma_synth_contig_bases(uint64_t seed, const int64_t* offsets, int64_t n, int32_t n_rate, uint8_t* seq);
int karma_synth_n_genes(uint64_t seed, int64_t n_contigs, int32_t gene_max, int64_t* n_genes);
int karma_synth_genes(uint64_t seed, int64_t n_contigs, int32_t gene_max, int64_t* gene_first, int32_t* gene_size);
/* Records of fragments [frag_lo, frag_hi): per-fragment record counts first
 * (rec_count[frag_hi-frag_lo]), then the records themselves. */
int karma_synth_read_counts(uint64_t seed, const int64_t* gene_first, const int32_t* gene_size, int64_t n_genes,
                            int64_t frag_lo, int64_t frag_hi, int paired, int32_t* rec_count);
int karma_synth_read_records(uint64_t seed, const int64_t* gene_first, const int32_t* gene_size, int64_t n_genes,
                             int64_t frag_lo, int64_t frag_hi, int paired, const int64_t* rec_off, uint32_t* records);
/* Salmon-style eq classes of fragments [frag_lo, frag_hi): each fragment's
 * deduplicated contig set, aggregated in order of first appearance (the
 * karma_graph_eq input).  cls_off == NULL: only *n_classes and *n_members. */
int karma_synth_eq_classes(uint64_t seed, const int64_t* gene_first, const int32_t* gene_size, int64_t n_genes,
                           int64_t frag_lo, int64_t frag_hi, int paired, int64_t* n_classes, int64_t* n_members,
                           int64_t* cls_off, uint32_t* members, int64_t* counts);

/* ---- host ingestion (C++, std::threads; no device needed) ----------------
 * Parsers over an in-memory file image, with Python text-mode semantics
 * (strict UTF-8, universal newlines).  Input the parser cannot reproduce
 * exactly (a malformed line, a non-ASCII integer, a duplicate eq name, ...)
 * returns KARMA_ERR_PARSE; the Python front end then raises the reference's
 * own exception.  threads <= 0: hardware concurrency. */
typedef struct karma_fasta karma_fasta;
/* read_fasta_file: records in OrderedDict order, keys with ">" kept.
 * seq: seq_bytes + 16 zero bytes of padding (the karma_contigs_create layout);
 * key_len in code points; ascii = 1 when every byte is < 0x80. */
int karma_fasta_parse(const char* data, size_t len, int threads, karma_fasta** out);
int karma_fasta_info(karma_fasta* f, int64_t* n, int64_t* seq_bytes, int64_t* key_bytes, int* ascii);
int karma_fasta_get(karma_fasta* f, uint8_t* seq, int64_t* seq_off, char* keys, int64_t* key_off,
                    int32_t* key_len);
/* Zero-copy view of the parsed arrays (valid until karma_fasta_destroy). */
int karma_fasta_view(karma_fasta* f, const uint8_t** seq, const int64_t** seq_off, const char** keys,
                     const int64_t** key_off, const int32_t** key_len);
int karma_fasta_destroy(karma_fasta* f);

typedef struct karma_eq karma_eq;
/* eq_classes.txt -> names + the karma_graph_eq arrays (cls_off[C+1], members,
 * counts, pair_skip = eq_size token == "1"). */
int karma_eq_parse(const char* data, size_t len, int threads, karma_eq** out);
int karma_eq_info(karma_eq* q, int64_t* n_contigs, int64_t* n_classes, int64_t* n_members, int64_t* name_bytes);
int karma_eq_get(karma_eq* q, char* names, int64_t* name_off, int64_t* cls_off, uint32_t* members, int64_t* counts,
                 uint8_t* pair_skip);
/* The same classes in the compact form karma_graph_eq_compact takes: sizes[C] =
 * member count | 0x80 when the eq_size token is "1", counts[C] as u32 (names,
 * name_off, members as karma_eq_get).  KARMA_ERR_ARG, nothing written, when a
 * class has more than 127 members or a count past 2^32 - 1. */
int karma_eq_get_compact(karma_eq* q, char* names, int64_t* name_off, uint8_t* sizes, uint32_t* members,
                         uint32_t* counts);
int karma_eq_destroy(karma_eq* q);

typedef struct karma_sam karma_sam;
/* SAM lines -> one (read id, contig id) record per line (the karma_graph_records
 * input, unsorted); contig ids number RNAMEs in order of first appearance, read
 * ids are an injective numbering of QNAMEs below read_id_bound.  q_start/q_len
 * locate each line's QNAME in the caller's buffer. */
int karma_sam_parse(const char* data, size_t len, int skip_headers, int threads, karma_sam** out);
int karma_sam_info(karma_sam* s, int64_t* n_records, int64_t* n_reads, int64_t* n_contigs, int64_t* rname_bytes,
                   int64_t* read_id_bound);
int karma_sam_get(karma_sam* s, uint32_t* records, char* rnames, int64_t* rname_off, int64_t* q_start,
                  int32_t* q_len);
int karma_sam_destroy(karma_sam* s);

/* ---- graph consumers --------------------------------
 * read_graph.py:150-172 (get_unconnected_nodes / get_connected_nodes),
 * :174-190 + :315-344 (node weights, representative sequences) and :350-357
 * (edge_list, MCL stdin), as karma.py:255-395 uses them on
 * ReadGraph(full_graph.subgraph(cluster)).  A karma_adj is a graph laid out as
 * networkx iterates it: nodes in iteration order (positions 0..n-1, each with an
 * id into the caller's name table) and per node its neighbours (positions) and
 * weights in adjacency-dict order. */
typedef struct karma_adj karma_adj;
/* add_edge(a[e], b[e], weight=w[e]) for e = 0..n_edges-1 on a graph whose n
 * nodes were added first (positions = ids order when ids == NULL). */
int karma_adj_from_edges(karma_ctx* ctx, int64_t n, const uint32_t* ids, const uint32_t* a, const uint32_t* b,
                         const double* w, int64_t n_edges, int is_device, karma_adj** out);
/* An exported adjacency: off[n+1] into nbr (positions) / w, in dict order. */
int karma_adj_from_lists(karma_ctx* ctx, int64_t n, const uint32_t* ids, const int64_t* off, const uint32_t* nbr,
                         const double* w, int is_device, karma_adj** out);
/* nx.Graph(G.subgraph(nodes)) of G = src: order[k] = distinct src positions in
 * the view's node order (host).  Adjacency rebuilt as from_dict_of_dicts does.
 * Stream-ordered: no host synchronisation. */
int karma_adj_view(karma_adj* src, const int64_t* order, int64_t k, karma_adj** out);
/* The consumers of a small view in one launch and one host synchronisation:
 * for nx.Graph(G.subgraph(nodes)) of G = src (order as karma_adj_view), deg[k]
 * (karma_adj_degrees), w[k] (karma_adj_node_weights) and, when with_text, the
 * edge_list text (karma_adj_edge_list; names / name_off on the device) into
 * text[text_cap].  *done = 0 (nothing computed) when the view exceeds one
 * block: k > 1024 nodes, > 4096 adjacency entries or text over text_cap (or
 * about 1 MB); the caller then takes karma_adj_view and the calls above. */
int karma_adj_view_summary(karma_adj* src, const int64_t* order, int64_t k, const uint8_t* names,
                           const int64_t* name_off, int with_text, int64_t* deg, double* w, uint8_t* text,
                           int64_t text_cap, int64_t* text_len, int* done);
/* G.remove_nodes_from: keep[n] (host, 1 = stays), n_keep = ones in keep;
 * remaining orders unchanged.  No host synchronisation. */
int karma_adj_keep(karma_adj* src, const uint8_t* keep, int64_t n_keep, karma_adj** out);
int karma_adj_info(karma_adj* g, int64_t* n, int64_t* n_entries);
/* Host copies of the layout (any pointer may be NULL). */
int karma_adj_get(karma_adj* g, uint32_t* ids, int64_t* off, uint32_t* nbr, double* w);
/* len(G.adj[u]) per position (nx.all_neighbors, a self-loop once). */
int karma_adj_degrees(karma_adj* g, int64_t* deg_host);
/* 0 + w_1 + w_2 + ... over G.adj[u] in order, f64 left to right (read_graph.py:183-187). */
int karma_adj_node_weights(karma_adj* g, double* w_host);
/* Both of the above in one pass (either pointer may be NULL). */
int karma_adj_node_stats(karma_adj* g, int64_t* deg_host, double* w_host);
/* "\n".join(f"{A} {B} {w}" for A, B, w in G.edges(data="weight")) as UTF-8:
 * names[name_off[i]:name_off[i+1]] is the UTF-8 name of id i; w is written as
 * Python repr(float).  out == NULL: only *len (the text is kept for the copying call). */
int karma_adj_edge_list(karma_adj* g, const uint8_t* names, const int64_t* name_off, int64_t n_names,
                        int names_on_device, uint8_t* out, int64_t cap, int64_t* len);
/* --rearrange (karma.py:103-118): sub[u] = subcluster
 * index of position u (-1: none; each node in at most one), rank[u] = its index
 * in that subcluster's node list.  For every pair A < B joined by an edge:
 * pair = A << 32 | B, sum = 0 + w_1 + w_2 + ... over the edges between them in
 * itertools.product(nodes_A, nodes_B) order, n_edges = their count, n_over = how
 * many of the partial sums exceed cutoff (the reference appends [A, B] once per
 * such edge); sorted by (A, B).  All outputs NULL: only *n_pairs. */
int karma_adj_cross_sums(karma_adj* g, const int32_t* sub, const int32_t* rank, double cutoff, uint64_t* pair,
                         double* sum, int64_t* n_edges, int64_t* n_over, int64_t cap, int64_t* n_pairs);
int karma_adj_destroy(karma_adj* g);
/* Host build of the device's repr(float) formatter, for tests: one line per value. */
int karma_repr_f64_host(const double* x, int64_t n, char* out, int64_t cap, int64_t* len);

/* ---- MCL: Markov clustering of a weighted graph -------------------------------
 * karma.py:317-318 and :372-373 pipe ReadGraph.edge_list() into the external
 * `mcl` binary (karma/mcl.py:48-51: -I <inflation> --abc -resource 4).  The
 * process below is defined here, bit for bit; equality with the binary's
 * clusters is not claimed (its pruning -- cutoff, selection, recovery, pct --
 * is richer than "keep the R largest" and has a tie order of its own).  What
 * is kept is what -resource 4 is for, at most R entries per column, and MCL's
 * usual defaults: loops of the column's maximum, inflation 2, cutoff 1/4000.
 *
 * Input: a graph as CSR in karma_adj_get's layout, off int64[n + 1], nbr
 * uint32[nnz], w f64[nnz] (nnz = off[n]), on the host or the device; rows need
 * not be sorted.  Column j of the matrix is CSR row j (no difference for the
 * symmetric graphs of a karma_adj).  1 <= n < 2^31, nnz < 2^31, 2 <= resource
 * (R) <= 32, 1.0 < inflation <= 16.0, 2^-40 <= cutoff <= 0.5, 0 <= eps,
 * max_iter >= 1, weights finite and > 0.
 *
 * Start.  Column j's entries are those with i = nbr[e] != j, value w[e];
 * entries naming j itself are ignored; the same i twice in one column is
 * KARMA_ERR_ARG.  The loop (j, m) is added, m the column's largest value, or
 * 1.0 for an empty column.  Entries ordered by row ascending; s = their
 * in-order sum from +0.0; T[i, j] = v / s.
 *
 * Iteration t = 1, 2, ...: every column j independently, on the previous T;
 * every step one IEEE f64 operation, no contraction.
 *   expand   for k over column j's rows ascending and i over column k's rows,
 *            the candidate p = T[i, k] * T[k, j]; X[i] = the sum of its
 *            candidates in ascending k from +0.0.
 *   prune    rows ordered by (X descending, i ascending); the first is kept;
 *            of the next R - 1 those with X[i] >= cutoff; s = the kept values'
 *            sum in ascending row order from +0.0; x = X / s.
 *   inflate  y = x * x when inflation == 2.0, else kpow(x, inflation) (the
 *            library's own, csrc/umap_math.h); s2 = the row-ascending sum of
 *            the y from +0.0; z = y / s2 is the new T[i, j].  Within the limits
 *            above every z > 0: x >= 2^-40 / 33 and inflation <= 16 keep y far
 *            above the smallest normal number.
 *   chaos    chaos_j = max_i z - (the row-ascending sum of z * z from +0.0);
 *            chaos = max_j chaos_j (an f64 maximum; a chaos_j may be a rounding
 *            error below zero, and is compared as it is).
 *   stop     after the first iteration with chaos < eps, or at t == max_iter.
 * A uniform clique converges in one iteration with all its members attractors
 * of one system (its R smallest members when it has more than R).  The result does not depend on block shape, path (general or
 * fused), batch size (cand_cap) or launch order.
 *
 * karma_mcl returns the final matrix as CSC: colptr int64[n + 1], rows
 * uint32 and vals f64 (each column ascending by row, at least one entry), in
 * buffers of cap >= n * resource entries (less: KARMA_ERR_ARG), on the host or
 * the device; *iterations and *chaos (host words) are those of the last
 * iteration run.  flags & KARMA_MCL_GENERAL: every iteration takes the general
 * path (sort-based, any column width; always used for iteration 1 and for
 * R > 8); otherwise iterations >= 2 run in one fused launch each.  cand_cap:
 * most candidates of one batch of the general path (whole columns; never less
 * than the widest column's count; 0: the default).  Argument errors
 * (KARMA_ERR_ARG, with a message) are found before a device is looked for; a
 * host graph's contents too; a device graph's contents by the first kernels,
 * before anything is indexed with them.  Timing-table names: mcl_start,
 * mcl_expand (general path), mcl_iter (fused path). */
#define KARMA_MCL_GENERAL 1
int karma_mcl(karma_ctx* ctx, int64_t n, const int64_t* off, const uint32_t* nbr, const double* w, int in_is_device,
              double inflation, int resource, double cutoff, double eps, int max_iter, int flags, int64_t cand_cap,
              int64_t* colptr, uint32_t* rows, double* vals, int64_t cap, int32_t* iterations, double* chaos,
              int out_is_device);
/* The same on a karma_adj's own device arrays: nothing is copied to the host. */
int karma_adj_mcl(karma_adj* g, double inflation, int resource, double cutoff, double eps, int max_iter, int flags,
                  int64_t cand_cap, int64_t* colptr, uint32_t* rows, double* vals, int64_t cap, int32_t* iterations,
                  double* chaos, int out_is_device);
/* The clusters of a final matrix (CSC, columns non-empty and ascending by
 * row), on the host: no device, no context.
 *   attractors  A = {a : T[a, a] present}.
 *   systems     the connected components of A under a ~ b when T[a, b] or
 *               T[b, a] is present.
 *   assignment  node j (attractors included) joins the system with the largest
 *               mass, a system's mass being the row-ascending sum from +0.0 of
 *               column j's entries on that system's attractors; ties go to the
 *               system whose smallest attractor is smallest.  A column with no
 *               entry on an attractor makes j a cluster of its own (possible
 *               only when max_iter stopped the run).
 *   labels      int32[n]: the rank of j's cluster under (size descending,
 *               smallest member ascending); *n_clusters their number. */
int karma_mcl_clusters(int64_t n, const int64_t* colptr, const uint32_t* rows, const double* vals, int32_t* labels,
                       int32_t* n_clusters);
/* For tests that place cases on the edges.  Fills the first n of v[0..3]:
 * columns per block of the fused kernel (resource <= 4), lanes per column for
 * resource <= 4 and for resource <= 8, the default cand_cap. */
int karma_mcl_tile(int* v, int n);

#ifdef __cplusplus
}
#endif
#endif /* KARMA_H */
