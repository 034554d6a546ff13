/*
 * vx_hash.h — C ABI of the MI355X SHA-1 piece-verification engine.
 *
 * This is the drop-in boundary for vortex's "Parallel hash computations" pool.
 * In the reference the boundary is not a trait but an inline closure handed to
 * rayon plus an mpsc channel back to the event loop:
 *
 *   submit   bittorrent/src/peer_comm/peer_connection.rs:1145-1158
 *            scope.spawn(move |_| { Sha1 over buffer[..piece_len];
 *                                   == metadata.pieces[index];
 *                                   complete_tx.send(DownloadedPiece{..}) })
 *   complete bittorrent/src/torrent.rs:415-442
 *            while let Ok(p) = downloaded_piece_rc.try_recv() { .. }
 *   bulk     bittorrent/src/torrent.rs:724-740 (par_iter over all pieces,
 *            each bittorrent/src/file_store.rs:228-303 check_piece_hash_sync)
 *   record   bittorrent/src/piece_selector.rs:311-317 (DownloadedPiece)
 *
 * Every entry point below names the reference interface it replaces.  The
 * signatures use only plain pointers, sizes and integers so that Rust
 * (`extern "C"`), ctypes, cgo or JNI can bind them directly; INTEGRATION.md
 * shows the Rust binding.
 *
 * Conventions
 *  - Return codes are 0 on success or a negative errno-style VX_E* value.  A
 *    hash mismatch is NOT an error: it is reported as matched = 0, exactly as
 *    the reference reports hash_matched = false.  No function aborts or throws
 *    across the ABI; vx_last_error() gives a thread-local message.
 *  - Digests are the 20-byte big-endian SHA-1 output (what
 *    `Sha1::finalize().as_slice()` returns), stored back to back.
 *  - Threading (mirrors the reference): one thread (the io_uring event-loop
 *    thread) submits and the same thread polls.  A vx_ctx is not internally
 *    synchronised; internal HIP streams are invisible to the caller.
 *    Separate contexts (e.g. one per torrent) share nothing but the device
 *    and may be driven from different threads concurrently
 *    (tests/test_gpu_parity.py::test_two_contexts_two_threads).
 *  - Device entry points (vx_sha1_device_*, vx_merkle_device_*) take device
 *    pointers and a HIP stream (hipStream_t passed as void*; NULL = the null
 *    stream) and only enqueue work: they return before the kernel finishes.
 *  - BitTorrent v2 (BEP 52) pieces are verified by the vx_merkle_* entries at
 *    the end of this file: 32-byte SHA-256 merkle roots in place of the
 *    20-byte digests, everything else as above.
 */
#ifndef VX_HASH_H
#define VX_HASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_ABI_VERSION 3

/* Error codes (negative errno values). */
#define VX_OK 0
#define VX_EINVAL (-22)  /* bad argument (null pointer, n/len out of range, misalignment) */
#define VX_ENOMEM (-12)  /* host or device allocation failed */
#define VX_ERANGE (-34)  /* piece longer than the context's max_piece_len */
#define VX_ENODEV (-19)  /* no such HIP device */
#define VX_EDEVICE (-5)  /* a HIP runtime call failed (see vx_last_error) */
#define VX_EBUSY (-16)   /* operation not allowed while work is in flight */

#define VX_DIGEST_LEN 20

/* Device batch layout: piece bytes live in one device allocation; piece i
 * starts at base + offsets[i] (uniform batches: base + i*stride).  Piece
 * starts must be 16-byte aligned (the kernels load 16 bytes per lane);
 * lengths are arbitrary (0 .. 4 GiB-1). */

/* One completion, the C form of DownloadedPiece (piece_selector.rs:311-317):
 * `tag` is whatever the caller passed to vx_submit (vortex packs the piece
 * index and the ConnectionId into it), `matched` is hash_matched.  The Buffer
 * member has no C counterpart: the caller keeps the buffer and gets it back
 * by tag. */
typedef struct vx_completion {
    uint64_t tag;
    uint8_t matched;
    uint8_t digest[VX_DIGEST_LEN];
    uint8_t _pad[3];
} vx_completion;

/* Everything a caller may choose is here; the engine reads no environment
 * variables.  Start from vx_config_default() and change fields (ABI 2 added
 * the six after slot_bytes; vx_create rejects values outside their ranges,
 * chunk sizes above 1 GiB included). */
typedef struct vx_config {
    int32_t device;             /* HIP device ordinal                                   */
    uint32_t max_piece_len;     /* bytes; torrent piece_length (torrent.rs:344 pool size) */
    uint32_t batch_pieces;      /* launch a batch once this many pieces are queued      */
    uint32_t slots;             /* batches in flight (each has its own stream + arena)  */
    uint64_t slot_bytes;        /* device arena bytes per slot (>= max_piece_len)       */
    uint32_t zero_copy;         /* 1 (default): a batch whose pieces are all registered and 16-byte aligned is
                                 * hashed straight out of host memory; 0: such pieces are gathered into HBM first */
    uint32_t direct_io;         /* re-verify: 1 (default) reads uncached, 4 KiB-aligned ranges with O_DIRECT;
                                 * 0: every read through the page cache (vortex's own pread)                   */
    uint32_t batch_chunk;       /* host batches of long pieces: bytes per resumable round (default 65536,
                                 * multiple of 4096); 0: whole pieces per slot                                  */
    uint32_t verify_chunk;      /* re-verify: bytes per resumable round (multiple of 4096); 0 (default): chosen
                                 * per call, 256 KiB when one window holds every piece, else 128 KiB           */
    uint32_t verify_cold_chunk; /* re-verify of data not in the page cache: bytes per round (multiple of 4096);
                                 * 0 (default): as when cached                                                  */
    uint32_t verify_ramp;       /* re-verify: first and last rounds shrink to chunk / 2^(d+1), d = 0..5
                                 * (default 1; 0: no ramp)                                                      */
    uint32_t refuse_when_full;  /* (ABI 3) async submits: 0 (default) wait for the oldest batch when every slot
                                 * is in flight; 1: return VX_EBUSY instead, the piece NOT taken, so the event
                                 * loop never blocks and hands the piece to its own pool (the overflow)      */
} vx_config;

typedef struct vx_ctx vx_ctx;

/* ---- library ---------------------------------------------------------- */
int vx_abi_version(void);
const char* vx_last_error(void);
const char* vx_strerror(int code);
/* Number of HIP devices (0 when no GPU or no driver). */
int vx_device_count(void);
/* Fill *cfg with defaults for a torrent whose piece_length is max_piece_len. */
void vx_config_default(vx_config* cfg, uint32_t max_piece_len);

/* ---- context: replaces InitializedState's downloaded_piece_tx/rc pair and
 *      the rayon scope it feeds (torrent.rs:319-320, 333; event_loop.rs:385) */
int vx_create(const vx_config* cfg, vx_ctx** out);
/* Drains all in-flight work first (the reference's scope joins every spawned
 * hash before EventLoop::run returns, event_loop.rs:385-602), then frees.
 * On a failed context it waits for the device to stop (every stream) before
 * unregistering host buffers, so borrowed buffers are free once it returns. */
int vx_destroy(vx_ctx* ctx);

/* Pin and device-map a host range (e.g. a BufferPool's AnonymousMmap,
 * buf_ring.rs:24-42) so pieces inside it reach the GPU without an internal
 * pinned copy: any batch slot whose pieces are all registered and 16-byte
 * aligned — async, or a host batch of short pieces — is hashed by a kernel
 * that reads them over PCIe itself (zero-copy slots, vx_config.zero_copy);
 * host batches of long pieces pull them with one gather kernel per resumable
 * round.  Ranges must not overlap. */
int vx_register_host_buffer(vx_ctx* ctx, void* ptr, size_t len);
int vx_unregister_host_buffer(vx_ctx* ctx, void* ptr);

/* ---- async download path ---------------------------------------------- */
/* Replaces `scope.spawn(hash closure)` (peer_connection.rs:1145-1158).
 * Hashes data[0..len) and compares with expected[0..20).  The engine borrows
 * `data` until the completion carrying `tag` has been returned by vx_poll;
 * it never frees or keeps it afterwards.  Never blocks on the GPU unless every
 * slot is in flight, in which case it waits for the oldest batch (the
 * reference's spawn never refuses work either).
 *
 * Ownership rule (vx_submit and vx_submit_piece): the piece is taken iff the
 * call returns 0.  0 means exactly one completion carrying `tag` will come
 * from vx_poll, or, if the context fails later, the tag is one of the
 * vx_pending() pieces never returned (INTEGRATION.md "Device failure").  Any
 * negative return means the piece was NOT taken: no completion will ever
 * carry `tag`, and the caller hashes the piece elsewhere (vortex: the original
 * scope.spawn closure).  Per code:
 *   VX_EINVAL   NULL context or data, or (vx_submit_piece) an index outside
 *               the piece table; the context is unchanged.
 *   VX_ERANGE   len > max_piece_len; the context is unchanged.
 *   VX_ENOMEM   the pinned stage for an unregistered piece could not be
 *               allocated; the context stays usable (a later submit may
 *               succeed, e.g. from a registered buffer).
 *   VX_EDEVICE  a launch failed (this call's batch-full launch, or the launch
 *               of the previous batch) or a batch failed while this call
 *               waited for a slot.  The context is dead from now on (every
 *               call returns the code); pieces taken earlier are recovered
 *               through vx_poll as documented there.  If this call's own
 *               batch launch failed part way, the device may still read
 *               `data` until vx_destroy returns.
 *   VX_EBUSY    (only with vx_config.refuse_when_full = 1) every slot is in
 *               flight and the open batch is full: the piece was NOT taken
 *               and nothing waited; hash it on the caller's pool.  Before
 *               refusing, the call may have launched the full open batch (the
 *               launch the next submit makes anyway; stats.batches + 1) and
 *               harvested finished batches without blocking (their results
 *               wait for vx_poll).  No piece changes owner: vx_pending() is
 *               the same before and after a refused call.
 * (VX_ENODEV is not returned by submits.) */
int vx_submit(vx_ctx* ctx, uint64_t tag, const uint8_t* data, uint32_t len, const uint8_t* expected);
/* Device-resident expected-digest table: upload the
 * torrent's `pieces` string (metadata.pieces, n_pieces x 20 B, the table the
 * closure indexes at peer_connection.rs:1146) once; vx_submit_piece then
 * names a row instead of passing 20 bytes per piece.  Replaces any previous
 * table; requires no pieces in flight. */
int vx_set_piece_table(vx_ctx* ctx, const uint8_t* table, uint32_t n_pieces);
/* vx_submit with expected = row piece_index of the piece table (same
 * ownership rule and return codes, VX_EBUSY under refuse_when_full included:
 * the full open batch may be launched and finished batches harvested before
 * the refusal, the refused piece is not taken). */
int vx_submit_piece(vx_ctx* ctx, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t piece_index);
/* Launch whatever is queued (call once per event-loop turn, next to the
 * drain at event_loop.rs:554-557).  If launching would leave no batch slot
 * free for the next vx_submit, the queued pieces stay open and keep
 * collecting, and the next vx_poll launches them once a batch completes:
 * under load batches grow instead of vx_submit blocking the loop thread. */
int vx_flush(vx_ctx* ctx);
/* Replaces `downloaded_piece_rc.try_recv()` (torrent.rs:418): non-blocking,
 * returns how many completions were written to out[0..max).  Order is the
 * order batches finish, which like the reference is not submission order.
 * Returns a negative VX_E* if a batch failed on the device.  After such a
 * failure the context is dead (every call returns the error), but vx_poll
 * still hands out the results of batches that did finish, and returns the
 * error only once none is left: the tags never returned are the pieces to
 * hash elsewhere (INTEGRATION.md "Device failure"), and vx_pending() is then
 * exactly their number. */
int64_t vx_poll(vx_ctx* ctx, vx_completion* out, size_t max);
/* Flush and block until every submitted piece has completed (results stay
 * queued for vx_poll).  timeout_ms = 0 waits forever. */
int vx_drain(vx_ctx* ctx, uint32_t timeout_ms);
/* Pieces submitted but not yet returned by vx_poll. */
uint64_t vx_pending(const vx_ctx* ctx);

/* ---- observability ------------------------------------------------------
 * vortex's hashing is invisible to its `metrics` feature (no
 * hash-time metric; the exported series are pieces_completed,
 * disk_write_time_ms, buffer_lifetime_ms ..., event_loop.rs:976-993,
 * buf_pool.rs:149-154).  These counters let the event loop export hash
 * throughput, mismatches, loop stalls and batch latency.  Cumulative since
 * vx_create or the last vx_reset_stats; host-side bookkeeping only (a clock
 * read per batch, none per piece).  Read them from the thread that drives the
 * context, like every other call. */
#define VX_STATS_HIST 24
typedef struct vx_stats {
    uint64_t pieces_completed;    /* results produced: async completions, host-batch and re-verified pieces */
    uint64_t pieces_mismatched;   /* of those compared with an expected digest, how many differed        */
    uint64_t bytes_completed;     /* piece bytes behind pieces_completed                                 */
    uint64_t batches;             /* whole-piece batches launched (async, host batches, re-verify slots) */
    uint64_t chunk_rounds;        /* resumable chunk rounds launched (long pieces)  */
    uint64_t gather_tiles;        /* 64 KiB tiles the gather kernel pulled from registered host buffers  */
    uint64_t staged_bytes;        /* bytes copied into pinned staging from unregistered caller memory    */
    uint64_t io_errors;           /* re-verified pieces with a failed or short read (torrent.rs:731-737) */
    uint64_t submit_stall_ns;     /* time submits waited for a batch to finish (the loop thread blocked) */
    uint64_t batch_latency_count; /* whole-piece batches harvested                                       */
    uint64_t batch_latency_sum_us; /* first submit of a batch -> its results harvested, summed           */
    uint64_t batch_latency_max_us;
    uint64_t batch_latency_hist[VX_STATS_HIST]; /* batches per [2^k, 2^(k+1)) us; [0] holds < 2 us, the last bucket everything longer */
    uint64_t zero_copy_slots;     /* (ABI 3) batches hashed straight out of registered host memory (§6.5)  */
    uint64_t zero_copy_loader_slots; /* (ABI 3) ... of them in the three-wave form (slots of < 128 pieces) */
    uint64_t submits_refused;     /* (ABI 3) async submits refused with VX_EBUSY (refuse_when_full)          */
} vx_stats;
int vx_get_stats(const vx_ctx* ctx, vx_stats* out);
int vx_reset_stats(vx_ctx* ctx);

/* Where the last vx_verify_files / _range call on ctx spent its time: the
 * startup re-verify's budget an operator sees (reads, PCIe copies, the tail).
 * Host times are steady-clock; copy times are the GPU's own (events around
 * each data H2D) and exist only on the resumable chunk path (pieces >= 2
 * chunks). */
typedef struct vx_verify_trace {
    double wall_ms;        /* the whole call                                          */
    double read_busy_ms;   /* pread time summed over the reader threads               */
    double read_span_ms;   /* first read started -> last read finished                */
    double first_read_ms;  /* call start -> first read finished (nothing overlaps it) */
    double copy_busy_ms;   /* GPU-timed data copies, summed (chunk path)              */
    double copy_span_ms;   /* first copy start -> last copy end, GPU clock            */
    double tail_ms;        /* last round enqueued -> verdicts on the host             */
    uint64_t read_bytes;   /* bytes pread                                             */
    uint64_t copy_bytes;   /* bytes of the timed copies                               */
    uint32_t readers;      /* reader threads                                          */
    uint32_t rounds;       /* timed copies (chunk rounds)                             */
    uint64_t direct_bytes; /* of read_bytes, read with O_DIRECT (not cached; §6.1)    */
    uint64_t chunk_bytes;  /* chunk of the resumable rounds (0: whole-piece slots)    */
} vx_verify_trace;
int vx_last_verify(const vx_ctx* ctx, vx_verify_trace* out);

/* The same call's round timeline (chunk path; none on the whole-piece path):
 * one record per round, in enqueue order, every time in ms from the call's
 * start on the host's steady clock.  GPU times are mapped onto it through an
 * event recorded on an idle stream at the call's start (error: that event's
 * dispatch latency, tens of us).  A gap on the copy engine between round k-1's
 * copy_end_ms and round k's copy_start_ms is the reads' when round k's
 * read_done_ms came after it, the hand-off's when its enqueue_ms did, and
 * otherwise the device's (stream dependencies). */
#define VX_ROUND_NEW_WINDOW 1u /* first round of a window of pieces              */
#define VX_ROUND_HEAD_RAMP 2u  /* a shortened round of the call's first chunk     */
#define VX_ROUND_TAIL_RAMP 4u  /* a shortened round of the call's last chunk      */
typedef struct vx_verify_round {
    double read_submit_ms; /* its reads queued on the reader pool                 */
    double read_done_ms;   /* its last read finished                              */
    double enqueue_ms;     /* its data copy and chunk kernel enqueued              */
    double copy_start_ms;  /* GPU: its data copy began (0 when not timed)         */
    double copy_end_ms;    /* GPU: its data copy ended                            */
    double kernel_end_ms;  /* GPU: its chunk kernel ended                         */
    uint64_t bytes;        /* bytes copied                                        */
    uint64_t offset;       /* the chunk's offset inside its pieces                */
    uint32_t lanes;        /* pieces in the round                                 */
    uint32_t flags;        /* VX_ROUND_*                                          */
} vx_verify_round;
/* Writes up to max records to out (may be NULL with max 0) and returns how
 * many rounds the call had. */
int64_t vx_last_verify_rounds(const vx_ctx* ctx, vx_verify_round* out, size_t max);

/* ---- skipping file holes in the re-verify -------------
 * The reference re-verifies right after it has fallocated every file to its
 * torrent length (file_store.rs:22-43, :146; torrent.rs:716-761), so what a
 * resume reads is mostly ranges no one ever wrote.  With on = 1 (default 0:
 * every call as before, nothing scanned) vx_verify_files, _range and _multi
 * and vx_merkle_verify_files and _range first ask the file system for each
 * opened file's data extents (lseek SEEK_DATA / SEEK_HOLE, at most 65,536 per
 * file; what lies beyond them is data) and judge what was never written
 * without reading it:
 *   v1  a piece whose every segment lies wholly in holes is not read, staged
 *       or copied; matched_out[i] = (expected row == SHA-1 of its length in
 *       zero bytes), that digest made once per context and length on the GPU.
 *       A piece only partly in holes is read whole, as before.
 *   v2  a 16 KiB block wholly in a hole is not read; its leaf row is the
 *       SHA-256 of its length in zero bytes, made on the GPU from nothing.  A
 *       piece's other blocks are read as before.
 *   hybrid  (vx_hybrid_verify_files / _range) the unit is the chunk of the
 *       call's rounds, 256 KiB (the piece where a piece is shorter than two
 *       chunks): a chunk whose data bytes all lie in holes is not read.  Its
 *       leaf rows are made as for v2; the SHA-1 chain crosses it on the GPU
 *       without zeros existing anywhere, and a piece with no written chunk is
 *       judged as a v1 hole piece is, over its data and implied pad.  A chunk
 *       only partly in holes is read whole; so is the trailing run of
 *       unwritten chunks of the torrent's last piece when that piece is
 *       shorter than piece_length (and not wholly unwritten).
 * A byte is a hole byte iff it lies below min(st_size, the file's torrent
 * length) and in no data extent: bytes past the end of a short file are
 * missing, not holes, so such a file fails the pieces it fails with the setting
 * off, and the return value counts them the same.  A file that did not open
 * has no holes; an lseek error other than ENXIO makes its whole file data.
 * Verdicts, return values and vx_get_stats are those of the setting off (hole
 * pieces count as completed, by their bytes, and as mismatched when they are);
 * vx_last_verify's read_bytes counts only what was read.
 * vx_verify_files_split (the pool claims pieces the engine cannot pre-judge)
 * and the three *_hash_files calls (a torrent is not created from unwritten
 * files) ignore the setting.  VX_EINVAL: NULL ctx, on not 0/1. */
int vx_set_skip_holes(vx_ctx* ctx, int on);
/* What the last vx_verify_files / vx_merkle_verify_files /
 * vx_hybrid_verify_files (or _range) call on ctx skipped; all zero when the
 * setting was off. */
typedef struct vx_hole_trace {
    uint64_t hole_pieces; /* v1, hybrid: pieces judged without a read              */
    uint64_t hole_blocks; /* v2, hybrid: 16 KiB blocks hashed from nothing (hybrid:
                             those of its hole pieces included)                    */
    uint64_t hole_bytes;  /* their bytes: not read, staged or copied               */
    uint64_t extents;     /* data extents the scan found, over all files           */
    double scan_ms;       /* the lseek scan and the classification                 */
    double zero_hash_ms;  /* GPU time of the zero hashes this call had to make
                             (0: every one came from the context's cache)          */
} vx_hole_trace;
int vx_last_verify_holes(const vx_ctx* ctx, vx_hole_trace* out);

/* ---- synchronous host batches (bulk re-verify, torrent.rs:724-740) ----- */
/* digests_out: n*20 bytes.  Pieces are pipelined through the slots, longest
 * first (ragged batches: DESIGN.md §6.4); outputs are always in the caller's
 * order.  Pieces may be of any lengths up to max_piece_len. */
int vx_sha1_batch(vx_ctx* ctx, const uint8_t* const* ptrs, const uint32_t* lens, size_t n, uint8_t* digests_out);
/* expected: n*20 bytes; matched_out: n bytes of 0/1 (the Box<[bool]> of
 * torrent.rs:727-740); digests_out may be NULL. */
int vx_verify_batch(vx_ctx* ctx, const uint8_t* const* ptrs, const uint32_t* lens, const uint8_t* expected,
                    size_t n, uint8_t* matched_out, uint8_t* digests_out);

/* ---- bulk re-verify from disk (torrent.rs:716-761, file_store.rs:228-303)
 * The torrent's files in order (path, length); the layout follows
 * FileStore::new (file_store.rs:126-160): pieces run across file boundaries,
 * piece i has piece_length bytes except the last (piece_selector.rs:63-69).
 * Every piece's segments are pread (io_threads readers, 0 = default) into
 * pinned batch buffers that stream to the GPU while the next batch is read.
 * matched_out[i] = 1 iff piece i was read completely and its SHA-1 equals
 * expected[20*i..].  A piece whose file is missing, short or unreadable is
 * matched = 0, like the reference's `Err(_) => false` (torrent.rs:731-737).
 * Returns the number of pieces that hit an I/O error (>= 0) or a VX_E* code.
 * Requires no async pieces pending on ctx. */
int64_t vx_verify_files(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                        uint32_t piece_length, const uint8_t* expected, size_t n_pieces, uint8_t* matched_out,
                        uint32_t io_threads);
/* Pieces [first, first+count) of the same torrent only: one rank's shard of a
 * multi-GPU re-verify (python: vortex_amd.shard.verify_files_sharded).
 * expected is still the whole n_pieces*20 table; matched_out has count
 * bytes, matched_out[k] for piece first+k.  Only that range's bytes are read.
 * vx_verify_files(...) is vx_verify_files_range(..., 0, n_pieces, ...). */
int64_t vx_verify_files_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                              uint32_t piece_length, const uint8_t* expected, size_t n_pieces, size_t first,
                              size_t count, uint8_t* matched_out, uint32_t io_threads);
/* ---- the self-balancing split (round 6) ---------------
 * One bulk re-verify shared at once by the engine and the caller's own pool
 * with no plan: torrent.rs:724-740's par_iter balances by rayon work
 * stealing, and this does the same across the PCIe boundary.  A vx_split is
 * one claim word over pieces [first, end): the pool takes pieces one by one
 * from the head (vx_split_claim, one compare-and-swap each), the engine takes
 * whole groups from the top as it forms its chunk rounds, and the two meet
 * wherever the host at hand puts them.  Before every round the engine
 * compares its remaining time with the pool's, both from rates measured in
 * this call (the pool's finished pieces per second through vx_split_done;
 * its own copy, read and per-block chain rates from the rounds' GPU events),
 * and takes the group of pieces that keeps the two finish times equal.
 * Its first group, before anything is measured, comes from the previous
 * split calls on the same context (their rates, and how far their finish
 * times strayed from the prediction), else from cpu_threads x
 * cpu_thread_rate and the PCIe rate.  The caller owns the struct; it may live
 * on the stack of the thread that starts both sides. */
typedef struct vx_split {
    uint64_t word;          /* head (low 32 bits) | stop (high 32): [head, stop) is unclaimed          */
    uint64_t pool_done;     /* pieces the pool finished (vx_split_done)                                */
    uint64_t start_ns;      /* steady clock at vx_split_init: the pool's rate is measured from here     */
    uint64_t first;         /* the range [first, end)                                                  */
    uint64_t end;
    uint32_t cpu_threads;   /* the pool's threads (0 = no pool: the engine takes every piece)          */
    uint32_t engines;       /* engines claiming at once (0 or 1: one; vx_verify_files_split_multi sets it) */
    double cpu_thread_rate; /* the pool's bytes/s per thread alone (cold start only; 0 = 2.2e9, SHA-NI) */
    uint64_t pool_last_ns;  /* steady clock at the pool's latest vx_split_done (when the pool finished)  */
} vx_split;
/* Pieces [first, end) unclaimed; end - first < 2^32 and end < 2^32. */
int vx_split_init(vx_split* s, uint64_t first, uint64_t end, uint32_t cpu_threads, double cpu_thread_rate);
/* Pool side, from any number of threads: the next piece from the head, or -1
 * when no piece is left for the pool.  After a piece's verdict is written,
 * call vx_split_done(s, 1): the engine reads the pool's rate from it. */
int64_t vx_split_claim(vx_split* s);
void vx_split_done(vx_split* s, uint64_t pieces);
/* The lowest piece the engine took (end when it took none): once both sides
 * have returned, the pool verified [first, boundary) and the engine
 * [boundary, end). */
uint64_t vx_split_boundary(const vx_split* s);
/* The engine's side: verifies the pieces it claims from s (always the top of
 * the range, contiguous) with resumable chunk rounds, while the caller's pool
 * runs vx_split_claim on its own threads; returns when its pieces are done.
 * If the pool has reported verdicts and is still working then, the engine
 * waits for it (polling, at most 3x its estimated remaining time + 50 ms) to
 * learn how far the two finish times strayed, for the next call's first
 * group; a pool that has reported nothing yet is not waited for, so a caller
 * may also run its pool after this returns.  With nothing in flight, the
 * engine takes the unclaimed pieces itself when the pool has finished none
 * for a while (two of its piece times, at least 4 ms): a pool busy elsewhere
 * does not leave them waiting.  matched_out has end - first bytes
 * (matched_out[k] for piece first + k); the engine writes only its own
 * pieces' entries, the pool writes the others.  Returns the number of the
 * engine's pieces that hit an I/O error (>= 0), or a VX_E* code: then the
 * pieces [vx_split_boundary(s), end) have no verdict and the caller verifies
 * them itself.  A split declared for one engine (engines 0 or 1) refuses a
 * second one with VX_EINVAL; with engines = k, k calls on k contexts may
 * claim from it at once (each engine's pieces are then its own groups, not
 * one tail).  Requires no async pieces pending on ctx.  vx_last_verify and
 * vx_last_verify_rounds describe the call as for vx_verify_files. */
int64_t vx_verify_files_split(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                              uint32_t piece_length, const uint8_t* expected, size_t n_pieces, vx_split* s,
                              uint8_t* matched_out, uint32_t io_threads);
/* The split over several GPUs of one process (one context per GPU, as for
 * vx_verify_files_multi) and the caller's pool at once: sets s->engines =
 * nctx and runs vx_verify_files_split on every context on its own host
 * thread, io_threads (the total) divided among them.  Returns the summed I/O
 * errors of the engines' pieces, or the first failing context's VX_E* code
 * (then re-verify [vx_split_boundary(s), end) on the pool: some of it has
 * verdicts, not all). */
int64_t vx_verify_files_split_multi(vx_ctx* const* ctxs, size_t nctx, const char* const* paths,
                                    const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
                                    const uint8_t* expected, size_t n_pieces, vx_split* s, uint8_t* matched_out,
                                    uint32_t io_threads);
/* In-process multi-GPU re-verify: vortex is one process with one event loop
 * (event_loop.rs:385), so on a multi-GPU host it holds one context per GPU
 * (vx_config.device) and hands them all to this call, which replaces the
 * whole par_iter of torrent.rs:724-740.  Pieces [0, n_pieces) are split into
 * nctx contiguous ranges (n_pieces/nctx each, the remainder to the last
 * contexts — the rule of vortex_amd.shard.shard_range) and context k verifies
 * range k on its own host thread with vx_verify_files_range, writing
 * matched_out[first_k ..] in place.  io_threads is the total reader count,
 * divided among the contexts (0 = default).  Contexts must be distinct and
 * idle; they may share a device.  Returns the summed I/O-error count, or the
 * first failing context's VX_E* code (vx_last_error names the context). */
int64_t vx_verify_files_multi(vx_ctx* const* ctxs, size_t nctx, const char* const* paths,
                              const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
                              const uint8_t* expected, size_t n_pieces, uint8_t* matched_out, uint32_t io_threads);

/* ---- planning: where should a bulk verify run? (host-only, no GPU) -----
 * One piece is one lane on the GPU and SHA-1 cannot be split inside a
 * piece, so a few very long pieces are bound by one lane's chain (~0.76 us
 * per 64-byte block, ~84 MB/s), while vortex's own rayon + `sha1` pool
 * (torrent.rs:724-740) hashes one piece per core at ~2 GB/s.  This cost model
 * (calibrated on MI355X) predicts both for n_pieces pieces of
 * piece_length bytes (total_length in all, the last piece shorter) read from
 * host memory or the page cache, so the caller can keep its own pool where it
 * is faster (INTEGRATION.md "Where the GPU pays").  cpu_threads / cpu_thread_rate
 * describe the caller's pool (0 = 16 threads / 2.2e9 B/s per thread, SHA-NI). */
typedef struct vx_plan {
    double gpu_s;               /* predicted e2e seconds of vx_verify_files / vx_verify_batch   */
    double gpu_chain_s;         /* one piece's chain of compressions in one lane               */
    double gpu_transfer_s;      /* all bytes over PCIe                                         */
    double cpu_s;               /* predicted seconds of the caller's pool                      */
    double piece_latency_s;     /* download path: submit-to-poll floor of one piece on the GPU */
    double cpu_piece_latency_s; /* the same piece on one pool thread                           */
    int32_t use_gpu;            /* 1 when 1.1 * gpu_s < cpu_s (near a tie, keep the CPU pool)  */
    uint32_t _pad;
} vx_plan;
int vx_plan_verify(uint64_t n_pieces, uint32_t piece_length, uint64_t total_length, uint32_t cpu_threads,
                   double cpu_thread_rate, vx_plan* out);
/* The same plan for a verify split over n_gpus contexts, one per GPU
 * (vx_verify_files_multi): gpu_transfer_s is each GPU's share over its own
 * link; gpu_chain_s, one piece's chain, does not shrink with more GPUs.
 * n_gpus 0 or 1 gives vx_plan_verify's answer. */
int vx_plan_verify_gpus(uint64_t n_pieces, uint32_t piece_length, uint64_t total_length, uint32_t cpu_threads,
                        double cpu_thread_rate, uint32_t n_gpus, vx_plan* out);
/* Split one bulk verify between the GPUs and the caller's own pool, both
 * running at once (torrent.rs:724-740's par_iter over the pool's range, and
 * vx_verify_files_range / _multi over the GPUs' range): the GPUs take the
 * contiguous tail [*gpu_first, n_pieces), *gpu_count pieces, chosen so the
 * predicted GPU time (the same model over n_gpus, its bytes at 0.74 of the
 * link: the pool shares host memory) meets the pool's time on the rest (at
 * 0.80 of cpu_thread_rate: the engine's readers share it too).
 * cpu_threads is the pool that runs beside the engine: leave the engine's
 * readers their cores (e.g. 12 pool threads beside 8 readers on 16 cores;
 * INTEGRATION.md "The split").  *gpu_count is 0 when no split beats the pool
 * alone by the 10 % margin, and n_pieces when the GPUs alone are fastest.
 * out (may be NULL) gets the plan of the split: gpu_s for the GPUs' range,
 * cpu_s for the pool's, use_gpu = 1 when the GPUs take part. */
int vx_plan_verify_split(uint64_t n_pieces, uint32_t piece_length, uint64_t total_length, uint32_t cpu_threads,
                         double cpu_thread_rate, uint32_t n_gpus, uint64_t* gpu_first, uint64_t* gpu_count,
                         vx_plan* out);

/* ---- device-resident batches (the hot path; no context needed) --------
 * These entries validate what they can see on the host — NULL pointers, the
 * alignment of d_base and stride, stride >= len — and nothing that lives in
 * device memory: d_offsets, d_lens and d_order are read only by the kernel,
 * so a misaligned or out-of-range offset, a length running past the
 * allocation or an order index >= n is NOT detected here and makes the
 * kernel read (or fault on) memory outside the batch.  Callers that build
 * the layout on the host check it there; the Python wrapper
 * vortex_amd.device.sha1_ragged checks it on the device before launching. */
/* Pieces i in [0,n) at d_base + i*stride, each len bytes.  Writes
 * d_digests[20*i..] (may be NULL) and, when d_expected is given,
 * d_matched[i] = (digest == d_expected[20*i..]) (0/1).  stride and d_base
 * must be multiples of 16 and stride >= len. */
int vx_sha1_device_uniform(const void* d_base, uint64_t stride, uint32_t len, uint32_t n, void* d_digests,
                           const void* d_expected, void* d_matched, void* stream);
/* Ragged batch: piece i at d_base + d_offsets[i] (16-byte aligned), d_lens[i]
 * bytes.  d_order (may be NULL) is a permutation of [0,n) telling lane j to
 * hash piece d_order[j]; pass pieces sorted by descending length so each
 * wavefront gets equal-length work (see vx_sort_order).  Runs the kernel
 * suited to chain-bound batches (lengths that differ). */
int vx_sha1_device_ragged(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                          const uint32_t* d_order, uint32_t n, void* d_digests, const void* d_expected,
                          void* d_matched, void* stream);
/* As vx_sha1_device_ragged, with the batch's longest piece and total bytes
 * (known on the host when the batch is laid out) so the engine picks the
 * kernel whose time bound, throughput or longest chain, is lower. */
int vx_sha1_device_ragged_hint(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                               const uint32_t* d_order, uint32_t n, uint32_t max_len, uint64_t total_len,
                               void* d_digests, const void* d_expected, void* d_matched, void* stream);
/* d_digests[20*j..] = SHA-1 of d_lens[j] zero bytes, j in [0,n): hashed from
 * nothing, no input is read but d_lens (4-byte aligned, as d_digests).  The
 * digest an unwritten piece's expected row is compared with (vx_set_skip_holes).
 * Enqueue-only; n == 0 launches nothing. */
int vx_sha1_device_zeros(const uint32_t* d_lens, uint32_t n, void* d_digests, void* stream);
/* Host helper: write into order_out the permutation that sorts lens[0..n)
 * by descending length (stable).  Used to build d_order. */
int vx_sort_order(const uint32_t* lens, uint32_t n, uint32_t* order_out);

/* ---- BitTorrent v2 (BEP 52): SHA-256 merkle piece verification ----------
 * A piece is a merkle tree over blocks of VX_MERKLE_BLOCK bytes, so it splits
 * across lanes where a SHA-1 piece is one chain.
 *   leaf      SHA-256 of one block; the last block of a piece at its real
 *             length (no zero fill).  A leaf slot wholly beyond the piece's
 *             bytes is the zero hash: 32 zero bytes, not the hash of anything.
 *   node      SHA-256(left || right).
 *   root      of a piece: the binary tree over width = 2^log2w leaf slots.
 *             Pieces of a file longer than piece_length (the short last one
 *             included) have width = piece_length / VX_MERKLE_BLOCK and their
 *             roots are the file's `piece layers`; a file of at most
 *             piece_length bytes is one piece whose width is its block count
 *             rounded up to a power of two and whose root is `pieces root`.
 *             An empty piece's root is the pad hash of its height.
 *   pad hash  pad(0) = the zero hash, pad(h) = SHA-256(pad(h-1) || pad(h-1)). */
#define VX_MERKLE_BLOCK 16384
#define VX_SHA256_LEN 32
#define VX_MERKLE_MAX_LOG2_WIDTH 17 /* 2^17 leaves: a 2 GiB piece */

/* Device-resident pieces i in [0,n) at d_base + i*stride, each len bytes, the
 * last one last_len (0 < last_len <= len); every tree has 2^log2_width leaf
 * slots (len <= VX_MERKLE_BLOCK << log2_width).  d_leaves (required,
 * (n << log2_width) * 32 bytes) receives every leaf row of every piece, zero
 * rows included: piece i's rows start at row i << log2_width; it is the leaf
 * layer a client serves to peers.  d_roots (n * 32 bytes, may be NULL) gets
 * the roots; with d_expected and d_matched both given, d_matched[i] =
 * (root == d_expected[32*i..]) (0/1).  d_base and stride are multiples of 16,
 * stride >= len, log2_width <= VX_MERKLE_MAX_LOG2_WIDTH and n << log2_width
 * fits 32 bits.  Enqueue-only, like the SHA-1 device entries; n == 0 launches
 * nothing. */
int vx_merkle_device_uniform(const void* d_base, uint64_t stride, uint32_t len, uint32_t last_len, uint32_t n,
                             uint32_t log2_width, void* d_leaves, void* d_roots, const void* d_expected,
                             void* d_matched, void* stream);
/* Ragged batch: piece i at d_base + d_offsets[i] (16-byte aligned), d_lens[i]
 * bytes (0 allowed).  d_log2w (uint8 per piece, may be NULL = log2_width)
 * gives piece i a tree of 2^d_log2w[i] <= 2^log2_width leaf slots (the single
 * piece of a short file); its leaf rows still start at row i << log2_width and
 * all 2^log2_width of them are written.  The device-resident metadata is not
 * checked here (see above); vortex_amd.device.merkle_ragged checks it. */
int vx_merkle_device_ragged(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint8_t* d_log2w, uint32_t n, uint32_t log2_width, void* d_leaves, void* d_roots,
                            const void* d_expected, void* d_matched, void* stream);
/* The same batch through the fused piece kernel, which keeps no leaf layer:
 * roots and verdicts only, the leaf rows live in LDS and never reach HBM (the
 * async path's kernel, vx_merkle_submit).  Arguments and checks as for
 * vx_merkle_device_ragged, with d_work in place of d_leaves:
 *   log2_width <= 8   one launch; d_work is unused and may be NULL.
 *   log2_width  > 8   d_work (16-byte aligned) holds T = n << (log2_width - 8)
 *                     rows of 32 bytes, the tops of the pieces' 256-leaf tiles
 *                     (piece i's at row i << (log2_width - 8)), followed by n
 *                     bytes, max(d_log2w[i] - 8, 0) per piece: T * 32 + n bytes
 *                     in all, written by the first launch and reduced by a
 *                     second (the node kernel at width log2_width - 8).
 * Enqueue-only; n == 0 launches nothing. */
int vx_merkle_device_pieces(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint8_t* d_log2w, uint32_t n, uint32_t log2_width, void* d_work, void* d_roots,
                            const void* d_expected, void* d_matched, void* stream);
/* Root of a layer of n hashes (32 bytes each) that stand `height` levels above
 * the leaves: the layer is padded to the next power of two with pad(height),
 * each level above with the next pad hash (how a client checks a received
 * `piece layers` string against `pieces root`).  d_work: 32*n bytes of
 * scratch; d_layer is not modified.  height <= 64. */
int vx_merkle_device_root(const void* d_layer, uint32_t n, uint32_t height, void* d_work, void* d_root,
                          void* stream);
/* pad(height) into out[32]; host only.  height <= 128. */
int vx_merkle_pad_hash(uint32_t height, uint8_t* out);
/* The synchronous host batch of v2 pieces, the counterpart of
 * vx_verify_batch: piece i is ptrs[i], lens[i] bytes (plain or registered
 * host memory), verified against expected[32*i..] as a tree of
 * 2^log2w[i] leaf slots (log2w NULL: piece_length / VX_MERKLE_BLOCK for
 * every piece).  matched_out[i] = 0/1; roots_out (may be NULL) gets n * 32
 * bytes.  Pieces go through the context's slots and pinned stages; one slot's
 * copy overlaps the previous slot's kernels.  piece_length is a power of two,
 * VX_MERKLE_BLOCK <= piece_length <= max_piece_len, and lens[i] <=
 * VX_MERKLE_BLOCK << log2w[i] <= piece_length.  VX_EBUSY while async pieces
 * are pending.  Counts into vx_get_stats (pieces_completed,
 * pieces_mismatched, bytes_completed, batches). */
int vx_merkle_verify_batch(vx_ctx* ctx, const uint8_t* const* ptrs, const uint32_t* lens, const uint8_t* log2w,
                           size_t n, uint32_t piece_length, const uint8_t* expected, uint8_t* matched_out,
                           uint8_t* roots_out);

/* The v2 download path: vx_submit / vx_poll for a BEP 52 piece.  One
 * completion; `root` is the piece's merkle root, `matched` = (root ==
 * expected) or 0 when the piece was submitted without one. */
typedef struct vx_merkle_completion {
    uint64_t tag;
    uint8_t matched;
    uint8_t root[VX_SHA256_LEN];
    uint8_t _pad[7];
} vx_merkle_completion; /* 48 bytes */
/* Queue data[0..len) as a v2 piece whose tree has 2^log2w leaf slots and
 * compare its root with expected[0..32) (NULL: the root is returned, matched
 * = 0).  len <= VX_MERKLE_BLOCK << log2w, and VX_MERKLE_BLOCK << log2w is at
 * most max_piece_len rounded up to a power of two (VX_EINVAL otherwise; len >
 * max_piece_len is VX_ERANGE).  Everything else is vx_submit's: the ownership
 * rule (the piece is taken iff the call returns 0), the return codes, VX_EBUSY
 * under refuse_when_full, the placement of registered and plain pieces.  v1
 * and v2 pieces share the context's batch slots, pending count, vx_flush,
 * vx_drain and statistics; a slot holds one kind, so a change of kind launches
 * the open batch.  A v2 slot is always copied or gathered into HBM first
 * (not hashed zero-copy unless vx_set_merkle_zero_copy) and hashed by the
 * fused piece kernel: one launch for trees of at most 256 leaves, two above. */
int vx_merkle_submit(vx_ctx* ctx, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t log2w,
                     const uint8_t* expected);
/* vx_poll for v2 pieces: vx_poll hands out v1 completions only, this call v2
 * only.  After a device failure each returns the results it still holds, then
 * the error. */
int64_t vx_merkle_poll(vx_ctx* ctx, vx_merkle_completion* out, size_t max);
/* Zero-copy for the v2 download path, off by default.  on = 1: a v2 slot whose
 * every piece lies in registered host memory at a 16-byte aligned address (what
 * makes a v1 slot zero-copy) is hashed by the zero-copy piece kernel straight
 * through the pieces' device mappings: no gather, no copy, no wait on the copy
 * chain, so the slot's PCIe transfer overlaps its own hashing.  Any other v2
 * slot takes the gathered path as with on = 0.  Roots, verdicts, completions
 * and vx_get_stats are the same either way (zero_copy_slots stays v1's, and
 * gather_tiles counts a zero-copy v2 slot's tiles as the gathered path would);
 * what the setting did is in the trace.  Read when a slot is launched, so it may
 * change while pieces are pending.  Hybrid slots, vx_merkle_verify_batch,
 * vx_merkle_check_blocks and the files calls do not look at it.
 * VX_EINVAL: NULL ctx, or on not 0/1. */
int vx_set_merkle_zero_copy(vx_ctx* ctx, int on);
/* Since vx_create: v2 slots launched zero-copy, their pieces and bytes, and v2
 * slots launched the gathered way while the setting was on.  (An unnamed
 * struct: the type is its typedef.) */
typedef struct {
    uint64_t slots, pieces, bytes, fallback_slots;
} vx_merkle_zc_trace;
int vx_merkle_zero_copy_trace(const vx_ctx* ctx, vx_merkle_zc_trace* out);

/* The two halves of the device entries on their own, for a caller that
 * streams blocks in rounds of its own (the re-verify below does).
 * Stage block b at d_stage + b*VX_MERKLE_BLOCK, d_lens[b] bytes; its leaf goes to row d_rows[b] of d_leaves
 * (0xFFFFFFFF: skipped; d_lens[b] == 0: the zero hash).  d_stage 16-byte aligned.
 * A block of length 0 or a skipped one is never read, so such entries may lie
 * past the end of the stage.  d_lens[b] <= VX_MERKLE_BLOCK and the rows are
 * device-resident and not checked here; vortex_amd.device.merkle_blocks
 * checks them.  Enqueue-only; n_blocks == 0 launches nothing. */
int vx_merkle_device_blocks(const void* d_stage, const uint32_t* d_rows, const uint32_t* d_lens,
                            uint32_t n_blocks, void* d_leaves, void* stream);
/* Reduce leaf rows that are already on the device: piece i's rows start at row i << log2_width, its tree has
 * 2^d_log2w[i] slots (NULL: log2_width).  roots / expected / matched as for vx_merkle_device_ragged. */
int vx_merkle_device_nodes(const void* d_leaves, const uint8_t* d_log2w, uint32_t n, uint32_t log2_width,
                           void* d_roots, const void* d_expected, void* d_matched, void* stream);
/* Leaf rows of unwritten blocks: row j of d_leaves (16-byte aligned) =
 * SHA-256 of d_lens[j] zero bytes, hashed from nothing.  d_lens[j] in
 * 1..VX_MERKLE_BLOCK is device-resident and not checked here;
 * vortex_amd.device.merkle_zero_leaves checks it.  Enqueue-only; n == 0
 * launches nothing. */
int vx_merkle_device_zero_leaves(const uint32_t* d_lens, uint32_t n, void* d_leaves, void* stream);

/* Re-verify a v2 torrent's files from disk: the v2 counterpart of
 * vx_verify_files.  Layout (BEP 52): every file starts its own pieces and no
 * piece spans files; pieces are numbered file by file in the order given; an
 * empty file has none; a file longer than piece_length has
 * ceil(len / piece_length) pieces of full width (expected rows: its `piece
 * layers`); a file of at most piece_length bytes is one piece as wide as its
 * block count rounded up to a power of two (expected row: its `pieces
 * root`).  n_pieces must equal that sum.  piece_length is a power of two from
 * VX_MERKLE_BLOCK to 2 GiB and is NOT bounded by max_piece_len or slot_bytes:
 * the files are streamed in rounds of 16 KiB blocks, cut wherever a slot's
 * stage is full, and only the finished 32-byte leaf rows are kept (in a device
 * window of 512 bytes x max(blocks per round, piece_length / 16 KiB)).
 * matched_out[i] = 1 iff every byte of piece i was read and its root equals
 * expected[32*i..]; a missing, short or unreadable file gives 0 for exactly
 * the pieces that lack bytes, and the return value counts those pieces (as
 * vx_verify_files).  io_threads 0 = a default.  VX_EBUSY while async pieces
 * are pending.  Counts into vx_get_stats and fills vx_last_verify
 * (chunk_bytes = a round's bytes); vx_last_verify_rounds returns 0. */
int64_t vx_merkle_verify_files(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                               uint32_t piece_length, const uint8_t* expected, size_t n_pieces,
                               uint8_t* matched_out, uint32_t io_threads);
/* Pieces [first, first + count) only, reading only their bytes (one rank's
 * shard); expected is the whole table, matched_out has count entries. */
int64_t vx_merkle_verify_files_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                     size_t nfiles, uint32_t piece_length, const uint8_t* expected, size_t n_pieces,
                                     size_t first, size_t count, uint8_t* matched_out, uint32_t io_threads);

/* ---- Hybrid (v1 + v2) torrents, BEP 52 "upgrade path" -------------------
 * One set of files carries a v1 `pieces` table (SHA-1) and v2 `piece layers` /
 * `pieces root` rows (SHA-256 merkle roots).  Every file but the last is
 * padded to a piece boundary with a BEP 47 pad file (attr = p, all zeros), so
 * every file starts its own pieces in v1 too: v1 piece i is v2 piece i (the
 * numbering of vx_merkle_verify_files), and the v1 piece that ends a file is
 * its data_len bytes followed by pad_len = piece_length - data_len zeros.  The
 * torrent's last piece (the last piece of the last non-empty file) has no pad.
 * Clients do not write pad files; these entries hash the zeros without reading
 * them from anywhere, and every data byte feeds both hashes from one copy.
 * A verdict byte has bit 0 set when the SHA-1 matches and bit 1 set when the
 * merkle root matches; 3 is a good piece, and 1 or 2 on bytes that were read
 * means the two tables disagree (BEP 52: reject the torrent).
 *
 * Device-resident batch: replaces vx_sha1_device_ragged over pieces with their
 * pads materialised, followed by vx_merkle_device_pieces over the same buffer.
 * Piece i is d_lens[i] bytes at d_base + d_offsets[i] (16-byte aligned) followed
 * by d_pads[i] implied zeros; d_pads[i] is 0 or (VX_MERKLE_BLOCK << log2_width)
 * - d_lens[i].  d_log2w, log2_width, d_roots and d_exp_roots as for
 * vx_merkle_device_pieces; d_sha1 (may be NULL) gets n * 20 bytes, d_exp_sha1
 * is n * 20 bytes.  With both expected tables NULL only digests and roots are
 * returned and d_matched is not written; with one NULL its bit stays clear.
 * d_work (16-byte aligned): W + 54 * n bytes, where W = 0 for log2_width <= 8
 * and the (n << (log2_width - 8)) * 32 + n bytes of vx_merkle_device_pieces
 * rounded up to 16 above (the chunk tables, the SHA-1 states and the two
 * verdict columns follow the merkle work).  Launches, on the caller's stream:
 * a table kernel, the chunked SHA-1 kernel over each piece's whole 64-byte
 * data blocks (a padded piece's state is kept), the zero-tail kernel over the
 * padded pieces, the merkle piece path, and a kernel that joins the verdicts.
 * The device-resident metadata is not checked here;
 * vortex_amd.device.hybrid_pieces checks it.  Enqueue-only; n == 0 launches
 * nothing. */
int vx_hybrid_device_pieces(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint32_t* d_pads, const uint8_t* d_log2w, uint32_t n, uint32_t log2_width,
                            void* d_work, void* d_sha1, void* d_roots, const void* d_exp_sha1,
                            const void* d_exp_roots, void* d_matched, void* stream);
/* Re-verify a hybrid torrent's files from disk in one pass: replaces
 * vx_verify_files over files plus materialised pad files followed by
 * vx_merkle_verify_files over the files.  paths / file_lengths list the real
 * files only, in torrent order with the pad files left out; pad files are
 * implied, never opened and never read.  exp_sha1 is the v1 `pieces` table
 * (n_pieces * 20 bytes), exp_roots what vx_merkle_verify_files takes
 * (n_pieces * 32 bytes), n_pieces the count of vx_merkle_verify_files.
 * matched_out[i] holds the two verdict bits; a missing, short or unreadable
 * file gives 0 for exactly the pieces that lack bytes (counted in io_errors).
 * Returns the number of pieces whose value is not 3, or a negative code.
 * Every byte is read once and copied to the device once: the files are
 * streamed in chunk rounds (chunk k of every piece of a window, as
 * vx_verify_files), each round's bytes feeding the chunked SHA-1 kernel and the
 * merkle block kernel.  piece_length is a power of two from VX_MERKLE_BLOCK to
 * 2 GiB and is not bounded by max_piece_len.  io_threads 0 = a default.
 * VX_EBUSY while async pieces are pending.  Counts into vx_get_stats
 * (pieces_mismatched once per piece that read well and is not 3) and fills
 * vx_last_verify (chunk_bytes = the chunk length); vx_last_verify_rounds
 * returns 0. */
int64_t vx_hybrid_verify_files(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                               uint32_t piece_length, const uint8_t* exp_sha1, const uint8_t* exp_roots,
                               size_t n_pieces, uint8_t* matched_out, uint32_t io_threads);
/* Pieces [first, first + count) only, reading only their bytes: replaces the
 * pair vx_verify_files_range / vx_merkle_verify_files_range.  The expected
 * tables are whole, matched_out has count entries. */
int64_t vx_hybrid_verify_files_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                     size_t nfiles, uint32_t piece_length, const uint8_t* exp_sha1,
                                     const uint8_t* exp_roots, size_t n_pieces, size_t first, size_t count,
                                     uint8_t* matched_out, uint32_t io_threads);

/* The hybrid download path: vx_submit / vx_poll for a piece of a hybrid
 * torrent.  One submit, one transfer and one completion give both hashes, in
 * place of vx_submit over a caller-made copy with the pad zeros appended plus
 * vx_merkle_submit, two slots and two completions to join.  `matched` holds the
 * verdict bits of the entries above (bit 0: SHA-1, bit 1: root; 3 = good). */
typedef struct vx_hybrid_completion {
    uint64_t tag;
    uint8_t matched;            /* bit 0: SHA-1 equal, bit 1: root equal */
    uint8_t _pad[3];
    uint8_t sha1[VX_DIGEST_LEN];  /* of data || pad_len zeros */
    uint8_t root[VX_SHA256_LEN];
} vx_hybrid_completion; /* 64 bytes */
/* Queue data[0..len), the piece's bytes on disk.  Its SHA-1 is taken over
 * those bytes followed by pad_len implied zeros (the BEP 47 pad behind a
 * file's last piece, hashed without being read from anywhere); its merkle tree
 * has 2^log2w leaf slots over data alone.  As vx_merkle_submit: len <=
 * VX_MERKLE_BLOCK << log2w, log2w <= VX_MERKLE_MAX_LOG2_WIDTH and the tree no
 * wider than max_piece_len rounded up to a power of two (VX_EINVAL); len >
 * max_piece_len is VX_ERANGE.  pad_len is 0, or len > 0 and len + pad_len is a
 * power of two >= VX_MERKLE_BLOCK, >= VX_MERKLE_BLOCK << log2w and <=
 * max_piece_len rounded up to a power of two (VX_EINVAL otherwise).
 * exp_sha1 (20 bytes) and exp_root (32 bytes) may each be NULL: a side's bit
 * is set iff that side was given and equal, exactly (a side not given is not
 * compared with anything); the digest and the root are always returned.
 * Everything else is vx_submit's: the ownership rule (the piece is taken iff
 * the call returns 0), every return code, VX_EBUSY under refuse_when_full, and
 * the placement (registered and 16-byte aligned: gathered; registered and
 * unaligned: copied straight from the caller's buffer; plain memory: through
 * the pinned stage).  v1, v2 and hybrid pieces share the context's batch
 * slots, pending count, vx_flush, vx_drain, the lazy flush, the sticky failure
 * and the statistics (pieces_mismatched counts a piece once when any compared
 * side fails, bytes_completed counts len).  A slot holds one kind, and within
 * the hybrid kind one padded total (len + pad_len of its padded pieces): a
 * change of either launches the open batch.  A hybrid slot is always copied or
 * gathered into HBM first (never hashed zero-copy) and both hashes read that
 * one copy: the merkle piece path runs on a stream of its own beside the SHA-1
 * kernel over the whole data blocks, and one kernel then finishes the padded
 * pieces' chains and compares both hashes. */
int vx_hybrid_submit(vx_ctx* ctx, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t pad_len,
                     uint32_t log2w, const uint8_t* exp_sha1, const uint8_t* exp_root);
/* Device-resident expected tables for hybrid pieces: the v1 `pieces` table
 * (n_pieces x 20 bytes) and the v2 rows (n_pieces x 32 bytes, in the numbering
 * of vx_hybrid_verify_files), uploaded once.  Replaces any earlier hybrid
 * tables, is independent of vx_set_piece_table, and requires no pieces in
 * flight (VX_EBUSY). */
int vx_hybrid_set_piece_tables(vx_ctx* ctx, const uint8_t* sha1_table, const uint8_t* roots_table,
                               uint32_t n_pieces);
/* vx_hybrid_submit with both expected rows = row piece_index of the hybrid
 * tables (both sides compared); an index outside the tables is VX_EINVAL.
 * Table-indexed and explicit pieces do not share a slot. */
int vx_hybrid_submit_piece(vx_ctx* ctx, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t pad_len,
                           uint32_t log2w, uint32_t piece_index);
/* vx_poll for hybrid pieces: vx_poll hands out v1 completions only,
 * vx_merkle_poll v2 only, this call hybrid only.  After a device failure each
 * returns the results it still holds, then the error.  Bulk calls return
 * VX_EBUSY while hybrid pieces are pending (the shared count). */
int64_t vx_hybrid_poll(vx_ctx* ctx, vx_hybrid_completion* out, size_t max);

/* ---- v2 metadata: `piece layers` and hash proofs in batches -------------
 * Every entry above takes its expected rows on trust.  BEP 52 says how a
 * client earns that trust: a file's `piece layers` string must reduce to the
 * file's `pieces root` (padded to a power of two with pad hashes), and a layer
 * that arrives over the wire comes in `hashes` messages, a span of consecutive
 * hashes of one layer followed by the uncle hashes that lead from the span's
 * root to `pieces root` or to an ancestor already trusted.
 *
 * Segmented layer roots: many layers of different sizes, all `height` levels
 * above the leaves (log2(piece_length / VX_MERKLE_BLOCK) for `piece layers`),
 * back to back in one buffer: layer f is counts[f] rows of 32 bytes.  The sizes
 * follow from the file lengths, so the host plans and the device only executes
 * (as for vx_sort_order).  A layer of m rows still alive at pass p is cut into
 * tiles of VX_MERKLE_TILE_ROWS rows, one workgroup each: m <= 512 is one last
 * tile of ceil(log2 m) levels whose top is the layer's root; otherwise every
 * tile reduces 9 levels (the short last tile filled with the pass's pad hash)
 * into a row of d_work, and those rows are the layer at pass p + 1.  Every
 * input row of pass p stands at height + 9p. */
#define VX_MERKLE_TILE_ROWS 512
typedef struct vx_merkle_tile { /* one workgroup in one pass; 16 bytes */
    uint32_t in_row; /* first input row: pass 0 a row of d_hashes, later passes a row of d_work        */
    uint32_t out;    /* last == 0: the row of d_work it writes; last == 1: the layer whose root this is */
    uint16_t rows;   /* 1..512 rows that exist; the tile is filled to 1 << levels with the pass's pad   */
    uint8_t levels;  /* 0..9 (0: the layer is one hash, its root is that hash)                          */
    uint8_t last;
    uint32_t _pad;
} vx_merkle_tile;
/* (No typedef: in C it would collide with the function of the same name, so
 * the struct is named by its tag, as `struct stat` beside stat().) */
struct vx_merkle_layers_plan {
    uint32_t n_layers, passes;       /* passes 0..4 */
    uint64_t rows;                   /* sum of counts */
    uint64_t work_rows;              /* 32-byte rows d_work must hold */
    uint32_t n_tiles, pass_tiles[4]; /* tiles of pass p lie consecutively, pass after pass */
    uint32_t _pad;
};
/* Plan n_layers layers of counts[f] >= 1 rows; host only.  tiles == NULL fills
 * *plan only, so the caller can size its buffers; otherwise tiles[0..n_tiles)
 * are written.  VX_EINVAL: a count of 0, a sum of counts of 2^32 or more, or
 * tiles given with tiles_cap < n_tiles (then nothing is written to tiles). */
int vx_merkle_layers_plan(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_layers_plan* plan,
                          vx_merkle_tile* tiles, size_t tiles_cap);
/* Execute a plan: plan->passes launches whatever n_layers is (n_layers == 0
 * launches nothing).  d_hashes: plan->rows rows, not modified; d_tiles: a
 * device copy of the planner's tiles; d_work: plan->work_rows rows (may be
 * NULL when that is 0).  d_roots (n_layers * 32 bytes, may be NULL) gets the
 * roots; with d_expected and d_matched both given, d_matched[f] = (root ==
 * d_expected[32*f..]).  height <= 64; d_hashes, d_work and d_roots 16-byte,
 * d_tiles and d_expected 4-byte aligned.  The tiles are device-resident and
 * not checked here.  Enqueue-only. */
int vx_merkle_device_layers(const void* d_hashes, const struct vx_merkle_layers_plan* plan,
                            const vx_merkle_tile* d_tiles, uint32_t height, void* d_work, void* d_roots,
                            const void* d_expected, void* d_matched, void* stream);

/* One `hashes` message (BEP 52), or the part of one a client checks at once:
 * `span` consecutive hashes of a layer and the uncles above them.  With
 * base layer 0 the span is a piece's leaf hashes and the result the piece's
 * row of `piece layers`: how a client finds the bad 16 KiB block of a failed
 * piece. */
typedef struct vx_merkle_proof { /* 24 bytes */
    uint64_t pos;      /* which span of its size in its layer (wire: index / length); bit k set: at step k the
                          running hash is the right child, node = H(uncle_k || cur); clear: H(cur || uncle_k) */
    uint32_t row;      /* first row of this proof in d_hashes: span rows, then uncles rows, as on the wire     */
    uint32_t expected; /* the row of d_expected the result must equal (many proofs share one root)             */
    uint16_t span;     /* a power of two, 1..512 */
    uint8_t uncles;    /* 0..64: the hashes behind the span in the message (its `proof layers` field is not used) */
    uint8_t _pad[5];
} vx_merkle_proof;
/* Verify n proofs in two launches: one workgroup per proof reduces its span to
 * the span's root (d_tops[32*i..], also the hand-over between the launches),
 * then one lane per proof walks the uncles, leaves the top in d_tops and sets
 * d_matched[i] = (top == d_expected[32 * expected..]).  d_tops (n * 32 bytes)
 * and d_matched (n bytes) are required.  The proofs are device-resident and
 * not checked here, but the kernels do not trust them: a span that is not a
 * power of two in 1..512 or uncles > 64 gives d_matched[i] = 0 and an all-zero
 * top, and none of that proof's rows are read.  row and expected are the
 * caller's to bound (vx_merkle_verify_proofs does).  d_hashes and d_tops
 * 16-byte, d_proofs 8-byte, d_expected 4-byte aligned.  Enqueue-only; n == 0
 * launches nothing. */
int vx_merkle_device_proofs(const void* d_hashes, const vx_merkle_proof* d_proofs, uint32_t n, void* d_tops,
                            const void* d_expected, void* d_matched, void* stream);

/* The two on a context, for hashes in host memory; both synchronous, on a
 * stream and device buffers of their own (allocated per call: this runs once
 * per torrent or per batch of messages, not per piece).  Neither touches the
 * batch slots, the pending count or vx_get_stats, and neither returns VX_EBUSY
 * while async pieces are pending: proofs for one file arrive while another
 * file's pieces download.
 * vx_merkle_verify_layers: hashes = the layers back to back (sum of counts
 * rows), expected = n_layers `pieces root` rows; matched_out[f] = 0/1;
 * roots_out (may be NULL) gets n_layers * 32 bytes. */
int vx_merkle_verify_layers(vx_ctx* ctx, const uint8_t* hashes, const uint32_t* counts, uint32_t n_layers,
                            uint32_t height, const uint8_t* expected, uint8_t* matched_out, uint8_t* roots_out);
/* vx_merkle_verify_proofs: hashes = n_rows rows holding every proof's span and
 * uncles, expected = n_expected trusted rows; matched_out[i] = 0/1; tops_out
 * (may be NULL) gets n * 32 bytes.  Each proof is checked first: span a power
 * of two of at most 512, uncles <= 64, row + span + uncles <= n_rows, expected
 * < n_expected; VX_EINVAL with the first bad index in vx_last_error. */
int vx_merkle_verify_proofs(vx_ctx* ctx, const uint8_t* hashes, uint64_t n_rows, const vx_merkle_proof* proofs,
                            uint32_t n, const uint8_t* expected, uint32_t n_expected, uint8_t* matched_out,
                            uint8_t* tops_out);

/* ---- Block checks: which 16 KiB blocks of a v2 piece are wrong -----------
 * A piece whose root is wrong says nothing about its blocks.  A client that
 * has the piece's leaf hashes (a `hashes` request at base layer 0, proven
 * against the piece-layer row it trusts with vx_merkle_verify_proofs) compares
 * every block with its leaf here and re-requests only the bad ones.  The same
 * calls return the leaf rows themselves: what a seeder answers such a request
 * from.
 *
 * The bitmap, a fixed contract: uint64 words, wpp = max(1, W / 64) words per
 * piece with W = 2^log2_width leaf slots; block b of piece i is bit b & 63 of
 * word i * wpp + (b >> 6); a set bit is a block whose SHA-256 differs from its
 * expected row.  A slot at or past the piece's end is never set, whatever its
 * expected row holds, and the bits of a word above W are 0.  Every word of
 * every piece is written, zeros included: the caller never clears it. */
/* Words of the bitmap of n pieces: n * max(1, 2^log2_width / 64); host only.
 * 0 when log2_width > VX_MERKLE_MAX_LOG2_WIDTH. */
uint64_t vx_merkle_bitmap_words(uint32_t n, uint32_t log2_width);
/* The batch of vx_merkle_device_ragged (every piece a tree of 2^log2_width
 * slots), checked block by block: leaf g = (i << log2_width) + b is compared
 * with row g of d_expected_leaves ((n << log2_width) * 32 bytes) into d_bad
 * (vx_merkle_bitmap_words(n, log2_width) words).  d_leaves_out (may be NULL)
 * gets the (n << log2_width) * 32 bytes vx_merkle_device_ragged writes to
 * d_leaves.  d_expected_leaves and d_bad are given together or both NULL (then
 * the call only writes d_leaves_out; all three NULL is VX_EINVAL).  d_base,
 * d_expected_leaves and d_leaves_out 16-byte, d_bad 8-byte aligned; n <<
 * log2_width fits 32 bits.  One launch, no atomics.  The device-resident
 * metadata is not checked here; vortex_amd.device.merkle_block_check checks
 * it.  Enqueue-only; n == 0 launches nothing. */
int vx_merkle_device_block_check(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t n,
                                 uint32_t log2_width, const void* d_expected_leaves, uint64_t* d_bad,
                                 void* d_leaves_out, void* stream);
/* The same on a context, for pieces in host memory (plain or registered):
 * piece i is ptrs[i], lens[i] bytes, a tree of W = piece_length /
 * VX_MERKLE_BLOCK slots.  expected_leaves (may be NULL): n * W rows of 32
 * bytes, piece i's at row i * W; bad_out: vx_merkle_bitmap_words(n,
 * log2(W)) words, required iff expected_leaves is given; bad_counts_out (may
 * be NULL, needs expected_leaves): per piece the number of set bits;
 * leaves_out (may be NULL): n * W * 32 bytes.  With expected_leaves and
 * leaves_out both NULL the call is VX_EINVAL.  piece_length is a power of two, VX_MERKLE_BLOCK <=
 * piece_length <= max_piece_len (VX_ERANGE above), lens[i] <= piece_length, no
 * NULL pointer for a non-empty piece; all of it is checked before anything is
 * allocated or copied.  Synchronous, on a stream and a device block of its
 * own as vx_merkle_verify_layers: the pieces go in rounds of at most
 * slot_bytes, copied from where they lie, one wait per round.  It touches
 * neither the batch slots, the pending count nor vx_get_stats and does not
 * return VX_EBUSY: a block check follows a failed piece in the middle of a
 * download, while async pieces are pending.  n == 0 returns 0. */
int vx_merkle_check_blocks(vx_ctx* ctx, const uint8_t* const* ptrs, const uint32_t* lens, size_t n,
                           uint32_t piece_length, const uint8_t* expected_leaves, uint64_t* bad_out,
                           uint32_t* bad_counts_out, uint8_t* leaves_out);

/* ---- Block checks from disk: the leaf table of a v2 torrent --------------
 * The torrent's leaf table is its files' leaf layers back to back, in file
 * order: file f contributes ceil(len_f / VX_MERKLE_BLOCK) rows of 32 bytes, an
 * empty file none, and there is no padding row anywhere.  Piece i (piece j of
 * file f, numbered as vx_merkle_verify_files numbers them) has
 * ceil(piece_len(i) / VX_MERKLE_BLOCK) rows from row
 *   leaf_off[f] + j * (piece_length / VX_MERKLE_BLOCK)
 * on, leaf_off[f] being the rows of the files in front of f.  The rows of a
 * range of pieces are one run of the table.  vx_merkle_hash_files_leaves
 * (below, with the hash calls) makes the table; a client keeps it with its
 * resume data and checks the files against it here.
 *
 * Rows of the whole table; host only, no context.  VX_EINVAL for a NULL
 * file_lengths or a piece_length that is not a power of two from
 * VX_MERKLE_BLOCK to 2 GiB. */
int64_t vx_merkle_leaf_rows(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length);
/* The kernel of the files calls on its own, on device-resident rows: n pieces
 * whose leaf rows lie piece-major in a window, piece k's 2^log2_width rows from
 * row row0 + (k << log2_width) on (all inside the window; 32-byte rows,
 * d_window 16-byte aligned).  Of piece k's rows the first d_blocks[k] (1 ..
 * 2^log2_width) are live and stand for rows d_leaf_first[k] .. of a compact
 * leaf table.
 *  - d_expected_leaves with d_bad (both or neither): each live row is compared
 *    with its row of that table; block b of piece k that differs is bit b & 63
 *    of word k * wpp + (b >> 6) of d_bad, the mapping of "The bitmap" above but
 *    with wpp words per piece as given, wpp >= max(1, 2^log2_width / 64).  The
 *    words (b >> 6) < max(1, 2^log2_width / 64) of every piece are written,
 *    zeros included; words above them are left as they are.  A dead slot is
 *    never set.
 *  - d_shadow_out (may be NULL; needs d_expected_leaves): a second window of
 *    the same rows; row row0 + (k << log2_width) + b gets the table's row of
 *    block b, 32 zero bytes for a dead slot: what vx_merkle_device_nodes
 *    reduces to tell whether the stored rows themselves belong to the piece.
 *  - d_leaves_out (may be NULL): the compact table to write; each live window
 *    row goes to its row of it.  Not the buffer d_expected_leaves names.
 * All three outputs NULL is VX_EINVAL.  n << log2_width fits 32 bits.  The
 * device-resident metadata is not checked here;
 * vortex_amd.device.merkle_leaf_check checks it.  One launch, no atomics.
 * Enqueue-only; n == 0 launches nothing. */
int vx_merkle_device_leaf_check(const void* d_window, uint32_t row0, uint32_t n, uint32_t log2_width, uint32_t wpp,
                                const uint32_t* d_leaf_first, const uint32_t* d_blocks,
                                const void* d_expected_leaves, uint64_t* d_bad, void* d_shadow_out,
                                void* d_leaves_out, void* stream);
/* vx_merkle_verify_files that also says which blocks are wrong, in the same
 * single pass over the files.  expected_leaves is the whole torrent's leaf
 * table and leaf_rows must equal vx_merkle_leaf_rows(...) (VX_EINVAL
 * otherwise, before anything is opened or allocated).  The return value,
 * matched_out, vx_get_stats, vx_last_verify, VX_EBUSY and vx_set_skip_holes
 * are exactly vx_merkle_verify_files'.  bad_out: vx_merkle_bitmap_words(
 * n_pieces, log2(piece_length / VX_MERKLE_BLOCK)) words in the mapping of "The
 * bitmap" above (every piece takes the full width's words, also the one piece
 * of a small file), every word written.  bad_counts_out[i] (may be NULL): the
 * set bits of piece i.  layer_ok_out[i] (may be NULL): 1 iff the stored leaf
 * rows of piece i reduce to expected[32*i..]; it does not depend on the data.
 * A piece that lacks bytes (missing, short or unreadable file) has matched 0
 * and every one of its existing blocks set.  The stored rows of the range are
 * held on the device for the call (1/512 of the range's bytes, VX_ENOMEM if
 * that cannot be had; the _range form bounds it); a range of 2^32 leaf rows or
 * more is VX_ERANGE.
 *
 *   matched  layer_ok  meaning
 *   1        any       the data is good; set bits can then only name stale
 *                      stored rows, and layer_ok is 0 if any is set
 *   0        1         the set bits are exactly the blocks to fetch again; at
 *                      least one bit is set
 *   0        0         fetch the piece, or fetch its leaf layer again first */
int64_t vx_merkle_verify_files_blocks(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                      size_t nfiles, uint32_t piece_length, const uint8_t* expected, size_t n_pieces,
                                      const uint8_t* expected_leaves, uint64_t leaf_rows, uint8_t* matched_out,
                                      uint8_t* layer_ok_out, uint64_t* bad_out, uint32_t* bad_counts_out,
                                      uint32_t io_threads);
/* Pieces [first, first + count) only: expected and expected_leaves are the
 * whole tables, of which only the range's rows are read; matched_out,
 * layer_ok_out and bad_counts_out have count entries, bad_out
 * vx_merkle_bitmap_words(count, log2(piece_length / VX_MERKLE_BLOCK)) words. */
int64_t vx_merkle_verify_files_blocks_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                            size_t nfiles, uint32_t piece_length, const uint8_t* expected,
                                            size_t n_pieces, const uint8_t* expected_leaves, uint64_t leaf_rows,
                                            size_t first, size_t count, uint8_t* matched_out, uint8_t* layer_ok_out,
                                            uint64_t* bad_out, uint32_t* bad_counts_out, uint32_t io_threads);

/* ---- Hashing: from files to `pieces`, `piece layers` and `pieces root` ---
 * Every entry above checks hashes that somebody else made.  The entries below
 * make them: what a client needs to create a torrent from a directory, and what
 * a seeder needs to answer BEP 52 hash requests.  Bencoding is the caller's.
 *
 * Layer trees.  Take a layer of m >= 1 rows of 32 bytes standing `height`
 * levels above the leaves, K = ceil(log2 m).  Its tree has levels k = 0..K;
 * level k holds n_k = ceil(m / 2^k) rows; level 0 is the layer; row j of level
 * k >= 1 is SHA-256(L || R) with L = row 2j of level k - 1 and R = row 2j + 1 of
 * level k - 1, or pad(height + k - 1) when that level has no such row.  Rows
 * that cover no row of the layer are pad hashes and are not stored.  The tree
 * is its levels back to back, level 0 first: vx_merkle_tree_rows(m) = sum of
 * n_k rows (at most 2m + K), the last of them the layer's root (what
 * vx_merkle_device_root and vx_merkle_device_layers give).  m = 1 is one row. */
uint64_t vx_merkle_tree_rows(uint64_t m);

/* One workgroup in one pass of vx_merkle_device_trees; 16 bytes, read as words.
 * The tile covers rows [512 * tile, 512 * tile + rows) of a level of level_rows
 * rows of one layer's tree, rows = min(512, level_rows - 512 * tile), and
 * reduces them by 9 levels when level_rows > 512 and by ceil(log2 level_rows)
 * otherwise. */
typedef struct vx_merkle_tree_tile {
    uint32_t src_row;    /* the level's first row where it is read: pass 0 a row of d_hashes, later = dst_row */
    uint32_t dst_row;    /* the level's first row in d_tree                                                  */
    uint32_t level_rows; /* rows of the level (pass p: level 9p of the layer's tree)                         */
    uint32_t tile;       /* which 512 rows of the level                                                      */
} vx_merkle_tree_tile;
struct vx_merkle_tree_plan {
    uint32_t n_layers, passes;       /* passes 0..4 */
    uint64_t rows;                   /* sum of counts: the rows of d_hashes */
    uint64_t tree_rows;              /* 32-byte rows d_tree must hold */
    uint32_t n_tiles, pass_tiles[4]; /* tiles of pass p lie consecutively, pass after pass */
    uint32_t _pad;
};
/* Plan the trees of n_layers layers of counts[f] >= 1 rows; host only.  The
 * pass rule is vx_merkle_layers_plan's.  tiles == NULL fills *plan only;
 * otherwise tiles[0..n_tiles) are written.  tree_off (may be NULL) gets
 * n_layers + 1 numbers: layer f's tree is rows [tree_off[f], tree_off[f + 1])
 * of d_tree, its root row tree_off[f + 1] - 1.  VX_EINVAL as
 * vx_merkle_layers_plan, and when the trees together hold 2^32 rows or more. */
int vx_merkle_tree_plan(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_tree_plan* plan,
                        vx_merkle_tree_tile* tiles, size_t tiles_cap, uint64_t* tree_off);
/* Execute a plan: plan->passes launches (n_layers == 0 launches nothing).
 * d_hashes: plan->rows rows, the layers back to back, not modified; d_tiles: a
 * device copy of the planner's tiles; d_tree: plan->tree_rows rows.  Pass 0
 * reads the layers and, in the same launch, copies each into level 0 of its
 * tree; pass p > 0 reads level 9p of every tree that reaches it from d_tree
 * itself, where pass p - 1 wrote it.  No workgroup reads a row that another
 * workgroup of the same launch writes.  There is no roots array: the root of
 * layer f is row tree_off[f + 1] - 1.  height <= 64; d_hashes and d_tree
 * 16-byte, d_tiles 4-byte aligned; d_tree must not overlap d_hashes.  The tiles
 * are device-resident and not checked here.  Enqueue-only. */
int vx_merkle_device_trees(const void* d_hashes, const struct vx_merkle_tree_plan* plan,
                           const vx_merkle_tree_tile* d_tiles, uint32_t height, void* d_tree, void* stream);
/* The same on a context, for layers in host memory (a client that has `piece
 * layers` from a .torrent and starts seeding): synchronous, on a stream and
 * device buffers of its own, as vx_merkle_verify_layers; it touches neither
 * the slots nor vx_get_stats and does not return VX_EBUSY while async pieces
 * are pending.  hashes = the layers back to back; tree_out = the trees back to
 * back (vx_merkle_tree_plan's tree_off; sum of vx_merkle_tree_rows(counts[f])
 * rows); roots_out (may be NULL) gets n_layers * 32 bytes. */
int vx_merkle_build_trees(vx_ctx* ctx, const uint8_t* hashes, const uint32_t* counts, uint32_t n_layers,
                          uint32_t height, uint8_t* tree_out, uint8_t* roots_out);
/* One `hashes` message out of a tree; host only, a pure lookup that hashes
 * nothing.  tree: the tree of an m-row layer at `height`.  Writes (span +
 * uncles) * 32 bytes to out in the row order of vx_merkle_proof: rows
 * [pos * span, (pos + 1) * span) of level `level`, then uncle t = row
 * (pos >> t) ^ 1 of level level + log2(span) + t.  A row at or past its level's
 * n_k, or of a level above K, is the pad hash of its height.  VX_EINVAL: span
 * not a power of two in 1..512, uncles > 64, level > K, height > 64, m == 0, or
 * pos * span >= n_level (a span without a row of the level).  Proofs at the
 * 16 KiB leaf level need the leaf layer, which the hash calls below do not
 * keep: vx_merkle_check_blocks with leaves_out returns a piece's, and its tree
 * (vx_merkle_build_trees at height 0) serves the rows inside the piece. */
int vx_merkle_tree_proof(const uint8_t* tree, uint32_t m, uint32_t height, uint32_t level, uint64_t pos,
                         uint32_t span, uint32_t uncles, uint8_t* out);

/* The trees of a v2 or hybrid torrent's files, host only: counts_out[f] (nfiles
 * numbers, may be NULL) is the rows of file f's layer: 0 for an empty file, 1
 * for a file of at most piece_length bytes (the row is its `pieces root`),
 * else its piece count (the rows are its `piece layers` entry, standing
 * log2(piece_length / VX_MERKLE_BLOCK) levels above the leaves).
 * tree_off_out (nfiles + 1 numbers, may be NULL): file f's tree is rows
 * [tree_off_out[f], tree_off_out[f + 1]) of tree_out below, empty for an empty
 * file; a non-empty file's `pieces root` is row tree_off_out[f + 1] - 1.
 * Returns the total rows, or VX_EINVAL (piece_length not a power of two from
 * VX_MERKLE_BLOCK to 2 GiB, a NULL file_lengths). */
int64_t vx_merkle_tree_layout(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
                              uint32_t* counts_out, uint64_t* tree_off_out);

/* Hash a v1 torrent's files into its `pieces` table: vx_verify_files without
 * an expected table (layout, readers and limits are that call's; the pieces
 * always stream as resumable chunk rounds).  digests_out[20*i..] is the SHA-1
 * of piece i; ok_out[i] (may be NULL) is 1 iff every byte of piece i was read.
 * A piece with ok == 0 has an all-zero digest.  Returns the number of pieces
 * that hit an I/O error, or a VX_E* code.  Common to the hash calls: VX_EBUSY
 * while async pieces are pending; they count into vx_get_stats
 * (pieces_completed, bytes_completed, batches or chunk_rounds as the verify
 * call of the same kind; pieces_mismatched is untouched) and fill
 * vx_last_verify as that verify call does. */
int64_t vx_hash_files(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                      uint32_t piece_length, size_t n_pieces, uint8_t* digests_out, uint8_t* ok_out,
                      uint32_t io_threads);
/* Pieces [first, first + count) only: digests_out has count * 20 bytes, ok_out
 * count bytes. */
int64_t vx_hash_files_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                            uint32_t piece_length, size_t n_pieces, size_t first, size_t count,
                            uint8_t* digests_out, uint8_t* ok_out, uint32_t io_threads);
/* Hash a v2 torrent's files: layout, numbering and limits are
 * vx_merkle_verify_files' (piece_length is not bounded by max_piece_len).
 * rows_out (n_pieces * 32 bytes) gets the rows that call takes as `expected`.
 * tree_out (may be NULL, then tree_rows is ignored) gets the layer trees of
 * every non-empty file in file order, as vx_merkle_tree_layout lays them out,
 * and tree_rows must equal that call's result (VX_EINVAL otherwise).  The trees
 * are built on the device from the call's own row table after the last round
 * and come back in one copy.  A piece with ok == 0 has an all-zero row, and a
 * file with any such piece has an all-zero tree: no tree is published over
 * bytes that were not read. */
int64_t vx_merkle_hash_files(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                             uint32_t piece_length, size_t n_pieces, uint8_t* rows_out, uint8_t* ok_out,
                             uint8_t* tree_out, uint64_t tree_rows, uint32_t io_threads);
/* Pieces [first, first + count) only; no tree. */
int64_t vx_merkle_hash_files_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                   size_t nfiles, uint32_t piece_length, size_t n_pieces, size_t first, size_t count,
                                   uint8_t* rows_out, uint8_t* ok_out, uint32_t io_threads);
/* vx_merkle_hash_files that also keeps the 16 KiB leaf layer, what a seeder
 * answers `hashes` requests at base layer 0 from and what
 * vx_merkle_verify_files_blocks checks against: leaves_out gets the whole
 * torrent's leaf table ("Block checks from disk" above) and leaf_rows must
 * equal vx_merkle_leaf_rows(...) (VX_EINVAL otherwise).  The rows of a piece
 * with ok == 0 are all zero: never a row over bytes that were not read.  The
 * table is held on the device until the last round and comes back in one copy
 * (VX_ENOMEM if it cannot be had, VX_ERANGE for 2^32 rows or more; the _range
 * form bounds it).  Everything else as vx_merkle_hash_files. */
int64_t vx_merkle_hash_files_leaves(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                    size_t nfiles, uint32_t piece_length, size_t n_pieces, uint8_t* rows_out,
                                    uint8_t* ok_out, uint8_t* tree_out, uint64_t tree_rows, uint8_t* leaves_out,
                                    uint64_t leaf_rows, uint32_t io_threads);
/* Pieces [first, first + count) only; no tree.  leaves_out is still the whole
 * table, of which only the range's rows are written. */
int64_t vx_merkle_hash_files_leaves_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                          size_t nfiles, uint32_t piece_length, size_t n_pieces, size_t first,
                                          size_t count, uint8_t* rows_out, uint8_t* ok_out, uint8_t* leaves_out,
                                          uint64_t leaf_rows, uint32_t io_threads);
/* Hash a hybrid torrent's files in one pass: vx_hybrid_verify_files with both
 * expected tables absent.  sha1_out[20*i..] is taken over piece i's data plus
 * its implied pad zeros, as that call defines it; rows_out, ok_out, tree_out
 * and tree_rows as for vx_merkle_hash_files. */
int64_t vx_hybrid_hash_files(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                             uint32_t piece_length, size_t n_pieces, uint8_t* sha1_out, uint8_t* rows_out,
                             uint8_t* ok_out, uint8_t* tree_out, uint64_t tree_rows, uint32_t io_threads);
int64_t vx_hybrid_hash_files_range(vx_ctx* ctx, const char* const* paths, const uint64_t* file_lengths,
                                   size_t nfiles, uint32_t piece_length, size_t n_pieces, size_t first, size_t count,
                                   uint8_t* sha1_out, uint8_t* rows_out, uint8_t* ok_out, uint32_t io_threads);

#ifdef __cplusplus
}
#endif
#endif /* VX_HASH_H */
