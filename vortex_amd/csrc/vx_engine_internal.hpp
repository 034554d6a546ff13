// vx_engine_internal.hpp — what every host unit of the engine shares (DESIGN.md
// "Host engine"): error reporting, the slot and context structs (one layout
// with and without VX_TEST_HOOKS), and the functions that cross units: the
// context's primitives (vx_engine.hip) and the slot path's (vx_slots.hip).
// Every device and pinned block, stream and event in them is a handle of
// vx_resources.hpp; the typed pointers beside them are views into the blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <unordered_map>
#include <numeric>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "vx_block_rounds.hpp"
#include "vx_extents.hpp"
#include "vx_files.hpp"
#include "vx_hash.h"
#include "vx_hybrid_slot.hpp"
#include "vx_kernels.h"
#include "vx_merkle_rounds.hpp"
#include "vx_merkle_tree.hpp"
#include "vx_resources.hpp"
#include "vx_synth.h"
#include "vx_tuning.h"

namespace vxe {

using vx_res::DeviceMem;
using vx_res::Event;
using vx_res::PinnedMem;
using vx_res::Stage;
using vx_res::Stream;

// the library's one error text per thread (vx_engine.hip): fail() writes it, vx_last_error reads it
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define VX_HIP(call)                                    \
    do {                                                  \
        hipError_t _e = (call);                           \
        if (_e != hipSuccess) return hip_fail(_e, #call); \
    } while (0)

constexpr uint64_t kAlign = 256;

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

struct Run {
    uint64_t lo, hi;  // staged byte range [lo, hi) of the arena
};

struct DirectRun {
    const uint8_t* host;  // registered (pinned) source of arena bytes [lo, hi)
    uint64_t lo, hi;
};

struct StageCopy {
    const uint8_t* src;  // unregistered caller bytes for stage [off, off + len)
    uint64_t off;
    uint32_t len;
};

// Movable (the context's vector of them), never copied.  Destroying a slot, or
// assigning Slot{} to it, gives back all it owns: first its stream (the last
// member), after waiting for it, then the blocks and events.
struct Slot {
    Event done;
    Event copied;  // this slot's H2D finished on the copy stream
    uint64_t arena_cap = 0;
    uint32_t cap = 0;  // pieces
    DeviceMem d_arena;
    Stage stage;  // the pinned stage, made on first use (ensure_stage)
    // pinned metadata block: offsets | lens | expected | digests | matched
    PinnedMem h_meta;
    DeviceMem d_meta;
    uint64_t* h_offsets = nullptr;
    uint32_t* h_lens = nullptr;
    uint8_t* h_expected = nullptr;
    uint8_t* h_digests = nullptr;
    uint8_t* h_matched = nullptr;
    uint32_t* h_pidx = nullptr;  // piece-table rows (vx_submit_piece) / piece ids (chunks)
    uint32_t* d_pidx = nullptr;
    uint64_t* h_poff = nullptr;  // chunked re-verify: chunk offset within its piece
    uint64_t* d_poff = nullptr;
    uint64_t* h_tlen = nullptr;  // chunked re-verify: the piece's total length
    uint64_t* d_tlen = nullptr;
    uint64_t* h_src = nullptr;   // gather: device-mapped source of piece i (0 = not gathered)
    uint64_t* d_src = nullptr;
    uint32_t* h_tfirst = nullptr;  // gather: piece i owns tiles [tfirst[i], tfirst[i+1])
    uint32_t* d_tfirst = nullptr;
    uint32_t gtiles = 0;           // gather tiles of this batch
    uint64_t* d_offsets = nullptr;
    uint32_t* d_lens = nullptr;
    uint8_t* d_expected = nullptr;
    uint8_t* d_digests = nullptr;
    uint8_t* d_matched = nullptr;
    // What the slot's pieces are (vx_submit / vx_merkle_submit / vx_hybrid_submit):
    // a slot holds one kind.  A slot filled by hand after reset_fill (the file
    // re-verify) is a v1 slot.
    enum class Kind : uint8_t { V1, V2, Hybrid };
    // v2 pieces, allocated on the slot's first v2 or hybrid use (ensure_v2): a
    // pinned block h and a device block d of expected roots (32 cap) | roots
    // (32 cap) | log2w (cap); the verdicts share h_matched / d_matched.
    struct V2 {
        PinnedMem h;
        DeviceMem d;
        uint8_t *h_exp32 = nullptr, *h_roots = nullptr, *h_log2w = nullptr;
        uint8_t *d_exp32 = nullptr, *d_roots = nullptr, *d_log2w = nullptr;
        // the piece kernel's work area for trees wider than 256 leaves (tile
        // tops | their log2w), grown when a launch needs more
        DeviceMem d_tops;
        uint32_t kmax = 0;  // the widest log2w of the slot's v2 or hybrid pieces: the piece kernel runs n << kmax lanes
    } v2;
    // hybrid pieces, allocated on the slot's first hybrid use (ensure_hybrid):
    // one pinned and one device block that hold a launch's whole metadata
    // (vx_hybrid_slot::Pack; the SHA-1 states behind it on the device), and the
    // event that joins the merkle side stream.  The roots land in the v2 block.
    // rows: what the submits filled in per piece, packed at launch.
    struct Hybrid {
        PinnedMem h;
        DeviceMem d;
        Event joined;
        struct Row {
            vx_hybrid_slot::Lane lane;
            uint8_t sha1[VX_DIGEST_LEN], root[VX_SHA256_LEN], log2w;
        };
        std::vector<Row> rows;
        uint64_t total = 0;  // the one padded total (len + pad_len) of the slot's padded pieces; 0: none yet
    } hy;
    std::vector<uint64_t> tags;
    std::vector<Run> runs;
    std::vector<DirectRun> druns;
    std::vector<StageCopy> staged;  // host batches: stage copies deferred to launch
    uint64_t staged_bytes = 0;
    uint32_t n = 0;
    uint64_t bytes = 0;
    bool uniform = true;
    bool has_expected = false;
    bool use_table = false;  // expected rows come from the device piece table(s), row h_pidx[i]
    Kind kind = Kind::V1;
    bool all_mapped = true;  // every non-empty piece is registered and 16-byte aligned (zero-copy candidate)
    enum State { FREE, FILLING, INFLIGHT } state = FREE;
    uint64_t seq = 0;
    std::chrono::steady_clock::time_point t_open{};  // first piece queued (vx_stats batch latency)
    // Declared last, so destroyed first: synchronized, then destroyed, before
    // any block above that a queued copy or kernel may still touch is freed.
    Stream stream;
};

}  // namespace vxe

// Ownership: every resource is a handle member and goes with
// `delete c`; a new one needs no line in vx_destroy.  Members go in reverse
// order, so each of the context's own streams (hy_stream, copy_stream, the
// holes') stands after the memory and the events its work uses, the slots
// included: it is synchronized and destroyed before they are freed.  The slot
// streams' work also uses blocks declared after the slots; every call waits
// for it before it returns, and vx_destroy waits for every stream before the
// members go.
struct vx_ctx {
    using DeviceMem = vx_res::DeviceMem;
    using PinnedMem = vx_res::PinnedMem;
    using Event = vx_res::Event;
    using Stream = vx_res::Stream;
    // Everything a caller chooses comes in here (vx_config, ABI 2): the
    // engine reads no environment variables.
    vx_config cfg{};
    std::vector<vxe::Slot> slots;
    // H2D copies are serialised across slots in launch order, so PCIe moves
    // one batch at a time at full rate and batch k's kernel starts as soon as
    // its own bytes are in, while batch k+1 copies (chain_h2d).  (Copies
    // racing on all slot streams share PCIe and delay every kernel.)
    int last_launched = -1;  // slot whose H2D was enqueued last
    // Per-piece device rows of the chunk paths (state | expected | digest |
    // verdict), kept across calls and grown on demand: allocating them per
    // call cost ~1 ms of a 40 ms e2e batch.
    DeviceMem d_chunk_rows;
    uint64_t chunk_rows_cap = 0;  // pieces
    Event chunk_prev;
    // Device-resident `pieces` table (vx_set_piece_table).
    DeviceMem d_table;
    uint32_t n_table = 0;
    int filling = -1;
    // vx_flush found every other slot in flight and left the filling slot
    // open; vx_poll launches it once a slot frees.
    bool flush_pending = false;
    bool bulk = false;  // inside vx_*_batch: slots fill to capacity, not to batch_pieces
    std::deque<vx_completion> done;
    std::deque<vx_merkle_completion> done_v2;  // v2 pieces' results (vx_merkle_poll)
    std::deque<vx_hybrid_completion> done_hy;  // hybrid pieces' results (vx_hybrid_poll)
    // vx_set_merkle_zero_copy: read by launch_v2 at every launch; what it did since vx_create
    int merkle_zc = 0;
    vx_merkle_zc_trace merkle_zc_trace{};
    // Hybrid download path: the device-resident v1 `pieces`
    // table and v2 rows (vx_hybrid_set_piece_tables), and the one side stream
    // every hybrid slot's merkle work runs on, beside the slot's SHA-1 chain;
    // created on the first hybrid launch.
    DeviceMem d_hy_sha1;
    DeviceMem d_hy_roots;
    uint32_t n_hy_table = 0;
    Stream hy_stream;
    struct Reg {
        size_t len;
        uint8_t* dev;  // device mapping of the range (hipHostGetDevicePointer)
    };
    std::map<uintptr_t, Reg> registered;
    // The same ranges keyed by start address: vortex submits each piece from
    // the start of its own pool mmap (buf_pool.rs:92-98), so most lookups are
    // one hash probe instead of a tree walk.  16 KiB pieces from 1,024
    // separately registered buffers: 29.7 -> 35.7 GiB/s.
    std::unordered_map<uintptr_t, Reg> registered_at;
    uint64_t pending = 0;
    uint64_t seq = 0;
    int sticky = 0;
    // Fault injection, used only in the test build libvortex_amd_tuning.so
    // (VX_TEST_HOOKS; always members, so every unit agrees on the layout).
    // vx_tuning_fail_submit_after: the submit after this many more succeeds
    // fails with VX_ENOMEM, the way a failed pinned-stage allocation does;
    // < 0 = off.
    int64_t fail_submit_after = -1;
    // vx_tuning_fail_launch_after: the launch after this many more fails as a
    // device error would, turning the context sticky; < 0 = off.
    int64_t fail_launch_after = -1;
    vx_stats stats{};  // vx_get_stats (observability counters)
    // harvest() counts mismatches unless the caller overrides verdicts after
    // it (the file re-verify: a piece with an I/O error is counted in
    // io_errors only, FileVerify::consume counts the final verdicts)
    bool harvest_counts_mismatches = true;
    // vx_last_verify: the last file re-verify's time budget, and the timing
    // events around its chunk rounds' data copies (reused across calls)
    vx_verify_trace last_verify{};
    std::vector<Event> copy_ev;
    std::vector<vx_verify_round> last_rounds;  // vx_last_verify_rounds
    // the last split call's decisions, one per round formed (vx_tuning_last_split)
    struct SplitDecision {
        double t_ms, pool_rate, engine_rate, block_ns, t_engine_ms, t_pool_ms;
        uint64_t unclaimed, group, lanes, pool_done;
        uint32_t mode, measured;
        double lag_ms;  // the learned lag in t_engine_ms
    };
    std::vector<SplitDecision> last_split;
    // What earlier split calls measured, the next call's cold start: the
    // engine's copy intake
    // (B/s, first copy start to last copy end), the kernel's chain per block,
    // and the pool's bytes/s per thread beside the engine (0 = none yet).
    // Each keeps the last kLearn calls' samples: the next call uses their
    // median (split_learn 1, default), so one call slowed by a host stall
    // does not move the next call's first group — and for the intake their
    // largest: a stall slows the pool as much as the engine's reads, and the
    // pool's side starts from its own rate alone, so the engine's starts from
    // its unstalled one too.  split_learn 0 (test build) uses the running mean
    // instead (each call weighted 1/2).
    struct Learned {
        static constexpr uint32_t kLearn = 5;
        double ring[kLearn] = {}, mean = 0;
        uint32_t n = 0;
        void add(double x) {
            mean = n ? 0.5 * (mean + x) : x;
            ring[n++ % kLearn] = x;
        }
        bool any() const { return n > 0; }
        double top() const { return *std::max_element(ring, ring + std::min(n, kLearn)); }
        double get(int median) const {
            if (!median) return mean;
            double v[kLearn];
            const uint32_t k = std::min(n, kLearn);
            std::copy(ring, ring + k, v);
            std::sort(v, v + k);
            return k % 2 ? v[k / 2] : 0.5 * (v[k / 2 - 1] + v[k / 2]);
        }
    };
    // [0]: calls over page-cached data, [1]: over uncached data (O_DIRECT
    // reads; the disk, not PCIe, feeds the engine): one regime's figures
    // would mislead the other's first group.
    Learned split_rin[2], split_bns[2], split_pool_thread_rate[2];
    int split_learn = 1;
    // How much later the engine's last kernel ended than the first group's
    // T_engine said, less the same for the pool's last verdict and T_pool, in
    // calls where the first group was the engine's only one (the readers'
    // start-up and the kernels trailing the copies, which the round model
    // leaves out), kept the same way; the next first group's T_engine adds
    // it.
    Learned split_lag[2];
    int split_lag_on = 1;  // 0: learned, not applied (vx_tuning_split_rules)
    // The file re-verify's chunk rounds put every H2D on this one stream (high
    // priority: its own hardware queue) and only kernels on the slot streams,
    // so no copy ever sits behind a kernel.  Created on first
    // use.  verify_copy_stream = 0 (test build only) restores the slot-stream
    // copies for A/B.
    Stream copy_stream;
    int verify_copy_stream = 1;
    // How pinned stages are allocated (Stage): 1 = 2 MiB-aligned mmap with
    // transparent huge pages, then registered; 0 = the pinned allocator
    // (vx_tuning_stage_huge, test build).  Huge pages: warm re-verify 39.1 ->
    // 45.2 GiB/s (its H2D copies 44-47 -> 49-50.5), cold 10.9 -> 14.2, median
    // of 7-9 alternating calls on one box.
    int stage_huge = 1;
    // The split's rules for pieces of one chunk (vx_tuning_split_rules, test
    // build): one_round 1 lets their groups keep claiming while the rates
    // are cold and skips the tenth rule (0: the multi-round rules; 2: as 1,
    // reading piece by piece instead of in runs);
    // round_cap > 0 caps their rounds' bytes (at no fewer than 1,024 lanes),
    // 0: the slot's stage.
    int split_one_round = 1;
    uint64_t split_round_cap = 64ull << 20;
    Event anchor_ev;  // maps the rounds' GPU times onto the host clock
    // vx_merkle_verify_batch: per slot, a device block (metadata in | results
    // out | leaf rows) and its pinned host mirror (in | out), allocated on the
    // first call; merkle_rows = leaf rows (and pieces) one round holds.
    struct MerkleBufs {
        DeviceMem d;
        PinnedMem h;
    };
    std::vector<MerkleBufs> merkle;
    uint32_t merkle_rows = 0;
    // vx_merkle_verify_files: the leaf-row window, per slot the pinned and
    // device rows | lens tables of a round, the per-call device rows
    // (expected | verdict | log2w per piece) and the event that orders one
    // round's kernels after the last round's; all kept across calls and grown
    // on demand.
    struct MerkleFiles {
        DeviceMem d_window;
        uint64_t window_rows = 0;
        std::vector<PinnedMem> h_tab;
        std::vector<DeviceMem> d_tab;
        uint64_t tab_entries = 0;
        DeviceMem d_call;
        uint64_t call_cap = 0;
        Event chain;
        // ... of the calls that keep or check the leaf layer (DESIGN.md §3.7
        // "Block checks from disk"): the range's rows of the leaf table, the
        // shadow window (the stored rows where the leaf window has the data's),
        // per piece leaf_first | blocks | layer_ok, and the range's bitmap.
        DeviceMem d_leaf;
        DeviceMem d_shadow;  // window_rows rows
        DeviceMem d_piece;
        uint64_t piece_cap = 0;  // pieces, 9 bytes each
        DeviceMem d_bad;
    } mfiles;
    uint64_t verify_t0_ns = 0;                // the running re-verify call's start (steady clock)
    // Skipping file holes in the re-verify (vx_set_skip_holes, DESIGN.md
    // §6.11): the setting, the last call's trace, and what the zero hashes need,
    // all made on first use: a stream of their own with two timing events, a
    // pinned block h and a device block d (kZeroBlock bytes each: 2 lengths |
    // 2 SHA-1 digests | one leaf row), the SHA-1 digests of zero pieces by
    // length (at most kZeroCache, the oldest dropped first) and the leaf row of
    // a full zero block.
    struct Holes {
        static constexpr size_t kZeroBlock = 128, kDigestsAt = 16, kLeafAt = 64, kZeroCache = 64;
        int skip = 0;
        vx_hole_trace last{};
        Event t0, t1;
        PinnedMem h;
        DeviceMem d;
        struct Sha1Zero {
            uint32_t len;
            uint8_t digest[VX_DIGEST_LEN];
        };
        std::vector<Sha1Zero> sha1_zero;
        uint8_t zero_leaf[VX_SHA256_LEN] = {};
        bool have_zero_leaf = false;
        Stream stream;  // after its events and blocks: waited for and destroyed before they go
    } holes;
};

namespace vxe {

// The GPU's per-block chain time on the split kernels and the PCIe rate: the
// cost model's hardware figures (vx_plan_verify), and the
// split's cold-start guesses before it has measured its own.
constexpr double kChainBlock = 0.76e-6, kPcieRate = 52.0 * (1ull << 30);

// The context's primitives (vx_engine.hip).
int set_device(const vx_ctx* c);
bool is_registered(const vx_ctx* c, const void* p, size_t len, const uint8_t** dev = nullptr);
unsigned usable_cpus();
int ensure_stage(const vx_ctx* c, Slot& s);
void reset_fill(Slot& s);
// The slot path (vx_slots.hip).
int chain_h2d(vx_ctx* c, int si);
void mark_launched(vx_ctx* c, int si);
int launch_slot(vx_ctx* c, int si);
int reap(vx_ctx* c, bool block_oldest);
bool zc_loader_wins(uint32_t n);
// What one submit brings.  expected: the row to compare with, or NULL for none
// (v1: a SHA-1 digest, v2: a root, hybrid: the SHA-1 row, exp_root its root);
// table: compare with row `row` of the device piece table(s) instead.
struct Piece {
    Slot::Kind kind;
    uint64_t tag;
    const uint8_t* data;
    uint32_t len;
    bool table = false;
    uint32_t row = 0;  // ... of the v1 table, or of the two hybrid tables
    const uint8_t *expected = nullptr, *exp_root = nullptr;
    uint32_t log2w = 0, pad_len = 0;  // v2 and hybrid: 2^log2w leaf slots; hybrid: implied zeros behind the data
};
int submit_impl(vx_ctx* c, const Piece& p);
void release_filling_slots(vx_ctx* c);   // every FILLING slot (reserved, never launched) back to FREE
void wait_and_free_inflight(vx_ctx* c);  // wait for every INFLIGHT slot, then free them unharvested
// A bulk call's guard: nothing pending (VX_EBUSY), not sticky, an empty filling
// slot handed back and, with need_idle, no slot in use ("a batch is in flight").
int begin_bulk_call(vx_ctx* c, const std::string& who, bool need_idle);

// A slot that is free now, after polling completions without blocking (on_reap
// runs after the poll); -1 in *si when there is none.
template <class F>
int try_free_slot(vx_ctx* c, int* si, F&& on_reap) {
    *si = -1;
    const int rc = reap(c, false);
    on_reap();
    if (rc) return rc;
    for (int k = 0; k < (int)c->slots.size() && *si < 0; ++k)
        if (c->slots[k].state == Slot::FREE) *si = k;
    return 0;
}
// A free slot, reaping the oldest in-flight one when none is; on_reap runs
// after every blocking reap.  none: the error when nothing is in flight either.
template <class F>
int free_slot(vx_ctx* c, const char* none, F&& on_reap) {
    for (;;) {
        bool inflight = false;
        for (int k = 0; k < (int)c->slots.size(); ++k) {
            if (c->slots[k].state == Slot::FREE) return k;
            inflight |= c->slots[k].state == Slot::INFLIGHT;
        }
        if (!inflight) return fail(VX_EDEVICE, none);
        int rc = reap(c, true);
        on_reap();
        if (rc) return rc;
    }
}
// free_slot (block) or try_free_slot into *si; the error, or 0 (*si < 0: none free now).
template <class F>
int take_slot(vx_ctx* c, bool block, const char* none, int* si, F&& on_reap) {
    if (!block) return try_free_slot(c, si, on_reap);
    *si = free_slot(c, none, on_reap);
    return *si < 0 ? *si : 0;
}

// The end of a file re-verify call (SHA-1 or merkle): what vx_last_verify
// reports of its readers; then the files closed, the wall time, and the
// call's result: rc, or the count of pieces with I/O errors (into vx_stats).
inline void trace_reads(vx_verify_trace& vt, vx_files::Readers& rd, const vx_files::DirectIo& dio, uint64_t t_call) {
    vt.read_busy_ms = rd.busy_ns() * 1e-6;
    vt.read_bytes = rd.bytes_read();
    vt.direct_bytes = dio.direct_bytes();
    vt.readers = (uint32_t)rd.threads();
    if (rd.first_start_ns()) {
        vt.read_span_ms = (rd.last_end_ns() - rd.first_start_ns()) * 1e-6;
        vt.first_read_ms = (rd.first_end_ns() - t_call) * 1e-6;
    }
}
inline int64_t end_files_call(vx_ctx* c, const std::vector<int>& fds, const std::vector<uint8_t>& bad,
                              uint64_t t_call, int rc) {
    for (int fd : fds)
        if (fd >= 0) close(fd);
    c->last_verify.wall_ms = (vx_files::Readers::now_ns() - t_call) * 1e-6;
    if (rc) return rc;
    int64_t nbad = 0;
    for (uint8_t x : bad) nbad += x;
    c->stats.io_errors += (uint64_t)nbad;
    return nbad;
}

// ---- The frame the v2 and the hybrid files call share (vx_merkle_files.hip, vx_hybrid.hip); a call
// keeps its buffers, what one round puts on the streams, its own stream syncs and its verdict fold. ----
// The argument checks (null_args: the caller's own NULL test of `names`), then begin_bulk_call.
inline int begin_block_call(vx_ctx* c, const std::string& who, bool null_args, const char* names,
                            const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length, size_t n_pieces,
                            size_t first, size_t count, uint64_t max_count, const uint8_t* tree_out,
                            uint64_t tree_rows) {
    if (!c) return fail(VX_EINVAL, who + ": NULL context");
    if (null_args) return fail(VX_EINVAL, who + ": NULL " + names);
    if (piece_length < VX_MERKLE_BLOCK || (piece_length & (piece_length - 1)))
        return fail(VX_EINVAL, who + ": piece_length must be a power of two >= 16384");
    if (n_pieces != vx_merkle::torrent_pieces(file_lengths, nfiles, piece_length))
        return fail(VX_EINVAL, who + ": n_pieces does not match the files");
    if (first > n_pieces || count > n_pieces - first) return fail(VX_EINVAL, who + ": piece range outside the torrent");
    if (count > max_count) return fail(VX_EINVAL, who + ": more than 2^32 pieces in one call");
    if (tree_out && (uint64_t)vx_merkle::tree_layout(file_lengths, nfiles, piece_length, nullptr, nullptr) != tree_rows)
        return fail(VX_EINVAL, who + ": tree_rows is not what vx_merkle_tree_layout returns");
    return begin_bulk_call(c, who, /*need_idle=*/true);
}
// VX_TEST_HOOKS: a round's injected failure, between its copies and its first kernel.
inline int injected_launch_failure(vx_ctx* c, const std::string& who) {
#ifdef VX_TEST_HOOKS
    if (c->fail_launch_after >= 0 && c->fail_launch_after-- == 0)
        return fail(VX_EDEVICE, who + ": injected launch failure (vx_tuning_fail_launch_after)");
#endif
    return 0;
}
// One call, made once its buffers exist: begin(), vx_block_rounds::run (this as
// the slots) over readers(), sync_slots(), the call's downloads, trace(), its fold, end().
struct BlockCall {
    vx_ctx* const c;
    const std::string& who;
    const size_t first, count;
    const uint64_t t_call = vx_files::Readers::now_ns();
    std::vector<int> fds;
    std::vector<uint8_t> bad;  // per piece of the range: it lacks bytes
    const std::vector<vx_files::FileSpan> no_spans;
    std::optional<vx_files::DirectIo> dio;
    std::optional<vx_files::Readers> rd;
    vx_block_rounds::Totals totals;
    ~BlockCall() {  // (a call that ended before end())
        for (int fd : fds)
            if (fd >= 0) close(fd);
    }

    // The files, ahead of begin() for a call that scans them first.
    void open_files(const char* const* paths, size_t nfiles) {
        fds.assign(nfiles, -1);
        for (size_t f = 0; f < nfiles; ++f) fds[f] = open(paths[f], O_RDONLY | O_CLOEXEC);
    }
    // The traces reset; behind the caller's copies of the expected tables
    // (tables_ok), the pieces' log2w column and the zeroed verdict bytes; then the files.
    int begin(bool tables_ok, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
              uint32_t piece_length, uint8_t* d_lw, uint8_t* d_verdicts, size_t verdict_bytes, uint8_t* matched_out) {
        c->last_verify = vx_verify_trace{};
        c->last_rounds.clear();
        c->verify_t0_ns = t_call;
        std::vector<uint8_t> lw(count);
        vx_merkle::PieceCursor pc(file_lengths, nfiles, piece_length);
        pc.seek(first);
        for (size_t i = 0; i < count; ++i, pc.next()) lw[i] = (uint8_t)pc.log2w();
        if (!tables_ok || hipMemcpy(d_lw, lw.data(), count, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(d_verdicts, 0, verdict_bytes) != hipSuccess ||
            hipStreamSynchronize(nullptr) != hipSuccess)  // (the slot streams do not wait for the null stream)
            return fail(VX_EDEVICE, who + ": expected-table upload failed");
        if (fds.empty()) open_files(paths, nfiles);
        bad.assign(count, 0);
        if (matched_out) std::memset(matched_out, 0, count);
        return 0;
    }
    // The readers of the rounds: runs of 16 KiB blocks, O_DIRECT where it pays.
    vx_files::Readers& readers(uint32_t io_threads, uint32_t piece_length) {
        dio.emplace(fds, c->cfg.direct_io != 0);
        return rd.emplace(io_threads ? (int)io_threads : (int)std::max(1u, std::min(16u, usable_cpus())), no_spans, fds,
                          piece_length, bad.data(), first, &*dio, true);
    }
    // The slots of vx_block_rounds::run: a slot's last round is done when its `done` event is.
    int done(size_t si, bool block) const {
        const Slot& s = c->slots[si];
        const hipError_t q = block ? hipEventSynchronize(s.done) : hipEventQuery(s.done);
        if (q == hipErrorNotReady) return vx_block_rounds::kNotYet;
        return q == hipSuccess ? 0 : fail(VX_EDEVICE, who + ": wait failed");
    }
    uint8_t* stage(size_t si, int* rc) const {
        *rc = ensure_stage(c, c->slots[si]);
        return c->slots[si].stage.get();
    }
    // After the rounds, error or not: no copy or kernel may still use a stage.
    void sync_slots(int& rc) const {
        for (const Slot& s : c->slots)
            if (s.stream && hipStreamSynchronize(s.stream) != hipSuccess && !rc)
                rc = fail(VX_EDEVICE, who + ": a round failed on the device");
    }
    // vx_last_verify, once the results are on the host.
    void trace(uint64_t chunk_bytes) {
        vx_verify_trace& vt = c->last_verify;
        vt.tail_ms = (vx_files::Readers::now_ns() - totals.last_enqueue_ns) * 1e-6;
        trace_reads(vt, *rd, *dio, t_call);
        vt.rounds = (uint32_t)totals.rounds;
        vt.copy_bytes = totals.copy_bytes;
        vt.chunk_bytes = chunk_bytes;
    }
    // vx_stats (mismatched: without the pieces that lack bytes, which end_files_call counts) and the result.
    int64_t end(int rc, uint64_t mismatched) {
        if (!rc) {
            c->stats.pieces_completed += count;
            c->stats.pieces_mismatched += mismatched;
            c->stats.bytes_completed += totals.file_bytes;
            c->stats.batches += totals.rounds;
        }
        rd.reset();
        dio.reset();
        const int64_t ended = end_files_call(c, fds, bad, t_call, rc);
        fds.clear();  // (closed)
        return ended;
    }
};

// Skipping file holes (vx_reverify.hip).  ensure_holes: the zero hashes'
// stream, events and blocks.  scan_holes: the files' extents when the setting
// is on (else an empty set, nothing scanned), counted and timed into the
// call's hole trace, which it resets.
int ensure_holes(vx_ctx* c, const char* who);
vx_extents::Holes scan_holes(vx_ctx* c, const std::vector<int>& fds, const uint64_t* file_lengths);
// vx_merkle_files.hip: the leaf row of a full unwritten block into c->holes.zero_leaf,
// made once per context; synchronous, on the holes' stream (so before a ZeroDigests::start).
int zero_leaf_row(vx_ctx* c, const char* who);

// The SHA-1 digests of zero pieces a call over file holes compares expected
// rows with (vx_verify_files and vx_hybrid_verify_files): at
// most two lengths per call, the torrent's piece length and its last piece's.
// start() launches sha1_zero_kernel for the lengths the context has not cached,
// on the holes' own stream, so the chain (a 2 MiB piece: 32,768 blocks, ~24 ms)
// runs beside the call's reads, copies and kernels; wait() takes the digests
// into the cache.  No host hashing: the product has none.
struct ZeroDigests {
    vx_ctx* c;
    const std::string who;
    vx_ctx::Holes::Sha1Zero have[2] = {};  // the call's lengths: cached ones first, then [n_have, n_have + n) launched
    int n_have = 0, n = 0;

    ZeroDigests(vx_ctx* ctx, const char* caller) : c(ctx), who(caller) {}
    const uint8_t* get(uint32_t len) const {
        for (int k = 0; k < n_have; ++k)
            if (have[k].len == len) return have[k].digest;
        return nullptr;
    }
    int start(const uint32_t* want, int nwant) {
        uint32_t lens[2] = {0, 0};
        for (int k = 0; k < nwant; ++k) {
            const auto& cache = c->holes.sha1_zero;
            const auto it = std::find_if(cache.begin(), cache.end(), [&](const auto& e) { return e.len == want[k]; });
            if (it != cache.end()) have[n_have++] = *it;
            else lens[n++] = want[k];
        }
        if (n == 0) return 0;
        for (int k = 0; k < n; ++k) have[n_have + k].len = lens[k];
        const int rc = ensure_holes(c, who.c_str());
        if (rc) return n = 0, rc;
        vx_ctx::Holes& h = c->holes;
        uint8_t *const hh = h.h.get(), *const hd = h.d.get();
        std::memcpy(hh, lens, sizeof(lens));
        hipError_t e = hipMemcpyAsync(hd, hh, sizeof(lens), hipMemcpyHostToDevice, h.stream);
        if (e == hipSuccess) e = hipEventRecord(h.t0, h.stream);
        if (e == hipSuccess)
            e = vx::launch_sha1_zeros(h.d.as<const uint32_t>(), (uint32_t)n, hd + h.kDigestsAt, h.stream);
        if (e == hipSuccess) e = hipEventRecord(h.t1, h.stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(hh + h.kDigestsAt, hd + h.kDigestsAt, (size_t)n * 20, hipMemcpyDeviceToHost, h.stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h.stream);
            return n = 0, hip_fail(e, (who + ": zero-piece digests").c_str());
        }
        return 0;
    }
    int wait() {
        if (n == 0) return 0;
        vx_ctx::Holes& h = c->holes;
        const int launched = n;
        n = 0;
        if (hipStreamSynchronize(h.stream) != hipSuccess)
            return fail(VX_EDEVICE, who + ": zero-piece digests failed on the device");
        float ms = 0;
        if (hipEventElapsedTime(&ms, h.t0, h.t1) == hipSuccess) h.last.zero_hash_ms += ms;
        for (int k = 0; k < launched; ++k) {
            vx_ctx::Holes::Sha1Zero& e = have[n_have++];
            std::memcpy(e.digest, h.h.get() + h.kDigestsAt + (size_t)k * 20, 20);
            if (h.sha1_zero.size() >= h.kZeroCache) h.sha1_zero.erase(h.sha1_zero.begin());
            h.sha1_zero.push_back(e);
        }
        return 0;
    }
};
// vx_merkle_files.hip, the end of a v2 or hybrid hash call: the layer trees of every
// non-empty file (vx_merkle_tree_layout) from d_rows, the whole torrent's piece
// rows on the device in piece order, into tree_out; synchronous, on st, with a
// device block of its own.  bad[i] != 0 (piece i lacks bytes) zeroes the tree
// of piece i's file.
int file_trees(vx_ctx* c, const uint8_t* d_rows, const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
               const std::vector<uint8_t>& bad, uint8_t* tree_out, hipStream_t st, const std::string& who);
// vx_reverify.hip, the _multi calls.  check_contexts: no NULL, no duplicate.
// fan_out: fn(k) for k in [0, nctx), one host thread per context (context 0,
// and any whose thread could not start, on the caller's); the sum of the
// results, or the first failing context's code, its error prefixed "context k: ".
int check_contexts(vx_ctx* const* ctxs, size_t nctx, const char* who);
int64_t fan_out(size_t nctx, const std::function<int64_t(size_t)>& fn);

}  // namespace vxe
