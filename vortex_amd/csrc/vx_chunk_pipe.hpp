// vx_chunk_pipe.hpp — the resumable chunk-round pipeline (ChunkPipe), its
// round schedule and the round timeline, shared by the chunked host batches,
// the file re-verify and the split; and what the latter two share.
#pragma once

#include "vx_engine_internal.hpp"

namespace vxe {

// One file re-verify call's verdict sink: completions never reach vx_poll.
struct FileVerify {
    vx_ctx* c;
    const uint8_t* expected;
    uint8_t* matched_out;
    std::vector<uint8_t>& bad;
    uint64_t done = 0;
    uint8_t* digests_out = nullptr;  // vx_hash_files: no expected table, the digests come back instead

    void consume() {
        while (!c->done.empty()) {
            const vx_completion& r = c->done.front();
            matched_out[r.tag] = (r.matched && !bad[r.tag]) ? 1 : 0;
            c->stats.pieces_mismatched += !r.matched && !bad[r.tag];  // I/O errors count in io_errors only
            c->done.pop_front();
            ++done;
        }
    }
    int slot(bool block, int* si) {  // take_slot, consuming after every reap
        return take_slot(c, block, "vx_verify_files: no slot to wait for", si, [this] { consume(); });
    }
};

// vx_verify_files_range, and with sp the engine's side of a split
// (vx_reverify.hip); verify_split is the split's driver (vx_split.hip).
int64_t verify_files_impl(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                          uint32_t piece_length, const uint8_t* expected, size_t n_pieces, size_t first,
                          size_t count, uint8_t* matched_out, uint32_t io_threads, vx_split* sp,
                          uint8_t* digests_out = nullptr);
int verify_split(FileVerify& fv, vx_files::Readers& rd, vx_split* sp, uint64_t n, uint32_t pl, uint64_t total,
                 uint64_t C, uint64_t* lowest, int regime);

// Re-verify reads run this many slots (whole pieces) or rounds (chunks)
// ahead of the one being enqueued, bounded by the slots.
constexpr size_t kReadahead = 2;

// Resumable chunk pipeline, shared by the file
// re-verify and strided host batches.  The call owns per-piece device rows
// (chaining state, expected digest, digest, verdict).  Each round is one slot:
// its H2D joins the copy chain across slots (chain_h2d), and its kernel waits
// for the previous round of the same window (state dependency) through
// `prev_kernel`, so PCIe moves round k+1 while the GPU compresses round k.
struct ChunkPipe {
    vx_ctx* c;
    uint64_t cnt = 0;
    uint64_t bytes = 0;  // the call's piece bytes (vx_stats)
    uint32_t* d_states = nullptr;
    uint8_t *d_exp = nullptr, *d_dig = nullptr, *d_match = nullptr;
    hipEvent_t prev_kernel = nullptr;
    bool have_prev = false;
    // Set (use_copy_stream): every round's H2D goes on the context's copy
    // stream, its kernel on the slot's stream after a wait on the round's
    // `copied` event.  Two slot streams can share one hardware queue (HIP maps
    // streams onto GPU_MAX_HW_QUEUES = 4), and a copy queued behind the other
    // slot's kernel there waited for that kernel: 5-7 ms of idle PCIe per
    // warm linux-mint call with 4-6 slots (profiles/r05/gaps/).
    hipStream_t cs = nullptr;
    // Set by a copy_data that records a timing event right after its copy on
    // the copy stream: the slot's stream waits on that one instead of a
    // separate `copied` marker (each marker between two copies on one stream
    // costs the copy engine ~15 us; 36 rounds of 8 MiB pieces add up).
    hipEvent_t copy_end = nullptr;
    // Set (the file re-verify over file holes): hole[i] != 0
    // marks a row no round hashes.  Its verdict byte is not the kernel's (the
    // caller overwrites it) and it is not counted here: the caller counts it.
    const uint8_t* hole = nullptr;

    explicit ChunkPipe(vx_ctx* ctx) : c(ctx) {}

    int use_copy_stream() {
        if (!c->copy_stream) {
            int least = 0, greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
                !c->copy_stream.make_with_priority(hipStreamNonBlocking, greatest))
                return fail(VX_EDEVICE, "chunk rounds: copy stream creation failed");
        }
        cs = c->copy_stream;
        return 0;
    }
    ~ChunkPipe() { release(); }
    ChunkPipe(const ChunkPipe&) = delete;
    ChunkPipe& operator=(const ChunkPipe&) = delete;

    // expected: count x 20 bytes or NULL (digests only).
    int open(uint64_t count, const uint8_t* expected, const char* who) {
        cnt = count;
        if (c->chunk_rows_cap < count) {  // kept across calls: grown only when too small, never reset
            const uint64_t grown = std::max<uint64_t>(count, 4096);
            c->chunk_rows_cap = c->d_chunk_rows.reserve(grown * 61 + 256) ? grown : 0;
            if (!c->chunk_rows_cap) return fail(VX_ENOMEM, std::string(who) + ": device allocation failed");
        }
        const uint64_t cap = c->chunk_rows_cap;
        uint8_t* const rows = c->d_chunk_rows.get();
        d_states = c->d_chunk_rows.as<uint32_t>();
        d_dig = rows + cap * 20;
        d_exp = expected ? rows + cap * 40 : nullptr;
        d_match = expected ? rows + cap * 60 : nullptr;
        if (!c->chunk_prev && !c->chunk_prev.make(hipEventDisableTiming))
            return fail(VX_EDEVICE, std::string(who) + ": event creation failed");
        prev_kernel = c->chunk_prev;
        if (expected && hipMemcpy(d_exp, expected, cnt * 20, hipMemcpyHostToDevice) != hipSuccess)
            return fail(VX_EDEVICE, std::string(who) + ": expected-table upload failed");
        return 0;
    }

    // A free slot, reaping the oldest round when none is (on_reap after each reap).
    template <class F>
    int free_slot(F&& on_reap) {
        return vxe::free_slot(c, "chunk rounds: no slot to wait for", on_reap);
    }
    // ... or, without block, one that is free now (-1 in *si: none): take_slot.
    template <class F>
    int slot(bool block, int* si, F&& on_reap) {
        return take_slot(c, block, "chunk rounds: no slot to wait for", si, on_reap);
    }

    // Slot si's h_offsets/h_lens/h_pidx/h_poff/h_tlen [0, m) describe the
    // round's lanes; copy_data(slot, stream) enqueues the chunk bytes into the
    // slot arena.  The lane table goes up as ONE copy of the metadata block's
    // head (offsets | chunk offsets | total lens | gather sources | lens |
    // piece rows, alloc_slot), not five: each small H2D is a blit kernel, and
    // five of them put ~0.1 ms between one round's data copy and the next.
    // When copy_data is a plain copy the table follows it, after `copied`, so
    // the next round's data copy (chained on `copied`) need not wait for it;
    // a gather (meta_first) reads d_offsets/d_lens, so the table goes first.
    // continues = the round follows one of the same window.
    //
    // With the copy stream (cs) the data copies go there, then `copied`; the
    // slot's stream takes the round's small lane table, waits for `copied`
    // and runs the kernel.  The data copies stay in launch order (one stream)
    // back to back, with no host wait and no small table copy between them
    // (on the copy stream each table added ~70 us to every round: 2.6 ms of
    // a 1,024 x 8 MiB call, profiles/r05/gaps/).  A table behind an aliased
    // slot's kernel only waits where the kernel waits anyway (the previous
    // round's state).  The slot is reused only after its `done` (free_slot),
    // so no copy overwrites a stage or arena a kernel still reads.
    template <class F>
    int round(int si, uint32_t m, bool continues, bool meta_first, F&& copy_data) {
        Slot& s = c->slots[si];
        hipStream_t st = s.stream;
        const size_t meta = (size_t)(reinterpret_cast<const uint8_t*>(s.h_pidx + m) - reinterpret_cast<const uint8_t*>(s.h_offsets));
        auto table = [&] {
            if (hipMemcpyAsync(s.d_offsets, s.h_offsets, meta, hipMemcpyHostToDevice, st) != hipSuccess)
                return fail(VX_EDEVICE, "chunk round: H2D failed");
            return 0;
        };
        int rc = 0;
        if (cs) {
            copy_end = nullptr;
            rc = copy_data(s, cs);
            hipEvent_t copied = copy_end ? copy_end : s.copied;
            if (!rc && copied == s.copied && hipEventRecord(s.copied, cs) != hipSuccess)
                rc = fail(VX_EDEVICE, "chunk round: event failed");
            if (!rc) rc = table();
            mark_launched(c, si);
            if (!rc && hipStreamWaitEvent(st, copied, 0) != hipSuccess)
                rc = fail(VX_EDEVICE, "chunk round: stream wait failed");
        } else {
            rc = chain_h2d(c, si);
            if (!rc && meta_first) rc = table();
            if (!rc) rc = copy_data(s, st);
            if (!rc && hipEventRecord(s.copied, st) != hipSuccess) rc = fail(VX_EDEVICE, "chunk round: event failed");
            if (!rc && !meta_first) rc = table();
            mark_launched(c, si);
        }
        return launch(s, m, continues, rc);
    }
    void end_window() { have_prev = false; }  // windows hold disjoint pieces

    // Wait for every round, then copy verdicts / digests back (either may be
    // NULL).  bad (may be NULL): pieces the caller fails for an I/O error,
    // counted in io_errors and not again as mismatches.
    int finish(uint8_t* matched_out, uint8_t* digests_out, int rc, const uint8_t* bad = nullptr) {
        return finish_rows(matched_out, rc, bad, {{0, cnt}}, digests_out);
    }

    // finish() for a set of row ranges (the split: this engine's claims):
    // verdicts back for those rows only, and only they count in vx_stats.
    int finish_rows(uint8_t* matched_out, int rc, const uint8_t* bad,
                    const std::vector<std::pair<uint64_t, uint64_t>>& rows, uint8_t* digests_out = nullptr) {
        if (!rc) {
            for (auto& s : c->slots)
                if (s.state == Slot::INFLIGHT && hipEventSynchronize(s.done) != hipSuccess) rc = VX_EDEVICE;
            if (rc) (void)fail(rc, "chunk rounds failed on device");
        }
        for (const auto& r : rows) {
            const uint64_t lo = std::min(r.first, cnt), hi = std::min(r.second, cnt);
            if (!rc && matched_out && d_match && hi > lo &&
                hipMemcpy(matched_out + lo, d_match + lo, hi - lo, hipMemcpyDeviceToHost) != hipSuccess)
                rc = fail(VX_EDEVICE, "verdict D2H failed");
        }
        if (!rc && digests_out && hipMemcpy(digests_out, d_dig, cnt * 20, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(VX_EDEVICE, "digest D2H failed");
        if (!rc) {
            c->stats.bytes_completed += bytes;
            for (const auto& r : rows) {
                c->stats.pieces_completed += r.second - r.first;
                for (uint64_t i = r.first; i < r.second && hole; ++i) c->stats.pieces_completed -= hole[i] != 0;
                if (matched_out && d_match)
                    for (uint64_t i = r.first; i < r.second; ++i)
                        c->stats.pieces_mismatched += matched_out[i] == 0 && !(bad && bad[i]) && !(hole && hole[i]);
            }
        }
        wait_and_free_inflight(c);
        return rc;
    }

    // The rows and the event belong to the context (they go with it);
    // only make sure nothing of this call is still running.
    void release() {
        if (cs) (void)hipStreamSynchronize(cs);  // data copies of this call's rounds
        for (auto& s : c->slots)
            if (s.stream) (void)hipStreamSynchronize(s.stream);
    }

private:
    // The part of round() both modes share: the round's kernel on the slot's
    // stream, after the previous round's of the same window, and the slot's
    // bookkeeping.  rc: what the mode's copies returned.
    int launch(Slot& s, uint32_t m, bool continues, int rc) {
        hipStream_t st = s.stream;
        if (!rc && continues && have_prev && hipStreamWaitEvent(st, prev_kernel, 0) != hipSuccess)
            rc = fail(VX_EDEVICE, "chunk round: stream wait failed");
#ifdef VX_TEST_HOOKS
        if (!rc && c->fail_launch_after >= 0 && c->fail_launch_after-- == 0)
            rc = fail(VX_EDEVICE, "chunk round: injected launch failure (vx_tuning_fail_launch_after)");
#endif
        if (!rc) {
            hipError_t e = vx::launch_chunk(s.d_arena.get(), s.d_offsets, s.d_lens, m, s.d_pidx, s.d_poff, s.d_tlen,
                                            d_states, d_dig, d_exp, d_match, st);
            if (e != hipSuccess) rc = hip_fail(e, "chunk kernel launch");
        }
        if (!rc && (hipEventRecord(prev_kernel, st) != hipSuccess || hipEventRecord(s.done, st) != hipSuccess))
            rc = fail(VX_EDEVICE, "chunk round: event record failed");
        have_prev = true;
        c->stats.chunk_rounds++;
        s.state = Slot::INFLIGHT;
        s.seq = c->seq++;
        s.n = 0;  // nothing to harvest: outputs live in the call's device rows
        if (rc) {
            // Part of the round may be queued (its data copy, on the copy
            // stream if there is one, the table on the slot's) while s.done
            // was not recorded for it (it may be stale): wait here, so no
            // later reuse or free of the stage and arena races a DMA of this
            // round.
            if (cs) (void)hipStreamSynchronize(cs);
            (void)hipStreamSynchronize(st);
        }
        if (!rc) rc = reap(c, false);
        return rc;
    }
};

// Round boundaries [a, a + len) over a window whose longest piece is L:
// chunks of C, and with `head`/`tail` ramps of depth d (q = C / 2^(d+1)) on
// the first / last C bytes: q, q, 2q, ..., C/2 up front and C/2, ..., 2q, q,
// rest (<= q) at the end, so the first read and the last chain — the parts
// of the pipeline nothing overlaps — shrink to q.  d = 1 is C/4, C/4, C/2.
// Every boundary is a multiple of q (>= 64 bytes for C >= 4 KiB, d <= 5), so
// no non-final chunk ends mid-block.
inline std::vector<std::pair<uint64_t, uint64_t>> chunk_schedule(uint64_t L, uint64_t C, int head, int tail) {
    std::vector<std::pair<uint64_t, uint64_t>> r;
    const int d = std::max(head, tail);
    const uint64_t q = C >> (d + 1);
    uint64_t a = 0;
    if (L == 0) r.push_back({0, 0});
    const bool ramp = d > 0 && q >= 64 && L >= 2 * C;  // head (ends at C) and tail (from >= C) never overlap
    if (ramp && head) {
        r.push_back({a, q});
        a += q;
        for (uint64_t len = q; len < C; len *= 2) r.push_back({a, len}), a += len;
    }
    // the tail ramp covers the last R bytes, R in (C - q, C]: C/2, ..., q, R - (C - q)
    const uint64_t tail_from = ramp && tail ? (L - C + q - 1) / q * q : L;
    while (a < tail_from) {
        const uint64_t len = std::min(C, tail_from - a);
        r.push_back({a, len});
        a += len;
    }
    if (a < L) {
        for (uint64_t len = C / 2; len >= q; len /= 2) r.push_back({a, len}), a += len;
        r.push_back({a, L - a});
        a = L;
    }
    return r;
}

// The round timeline of one file re-verify call (vx_last_verify /
// vx_last_verify_rounds).  Timing events around each round's data copy and
// after its kernel (start, end, kernel end: copy_ev[3k .. 3k+2]) are kept on
// the context and reused.  An anchor event recorded on an idle stream at the
// start maps GPU times onto the host clock of the call.
struct RoundTimeline {
    using clk = std::chrono::steady_clock;
    vx_ctx* c;
    ChunkPipe& cp;
    const std::string h2d_failed;  // the caller's "<who>: chunk H2D failed"
    size_t timed = 0;
    std::vector<uint64_t> timed_bytes;
    std::vector<vx_verify_round> tl;  // one per enqueued round
    std::vector<long> tl_ev;          // timed-copy index of each timeline round, -1 when untimed
    bool anchored = false;
    uint64_t t_anchor = 0;
    clk::time_point t_last_enqueue;
    long ev_k = -1;          // timed-copy index of the round being enqueued
    uint64_t t_enqueue = 0;  // ... and when its enqueue began (timed_copy)

    RoundTimeline(vx_ctx* ctx, ChunkPipe& pipe, const char* who)
        : c(ctx), cp(pipe), h2d_failed(std::string(who) + ": chunk H2D failed") {
        if (c->anchor_ev || c->anchor_ev.make(hipEventDefault)) {  // (timed)
            anchored = hipEventRecord(c->anchor_ev, c->slots[0].stream) == hipSuccess;
            t_anchor = vx_files::Readers::now_ns();
        }
        t_last_enqueue = clk::now();
    }
    double rel_ms(uint64_t t_ns) const { return t_ns ? ((double)t_ns - (double)c->verify_t0_ns) * 1e-6 : 0.0; }
    // cp.round's copy_data: one plain copy of the slot's stage, timed (best effort)
    auto timed_copy() {
        ev_k = -1;
        t_enqueue = vx_files::Readers::now_ns();
        return [this](Slot& sl, hipStream_t st) {
            bool ev = true;
            while (ev && c->copy_ev.size() < 3 * timed + 3) {
                Event e;
                ev = e.make(hipEventDefault);  // (timed)
                if (ev) c->copy_ev.push_back(std::move(e));
            }
            ev = ev && hipEventRecord(c->copy_ev[3 * timed], st) == hipSuccess;
            if (hipMemcpyAsync(sl.d_arena.get(), sl.stage.get(), sl.bytes, hipMemcpyHostToDevice, st) != hipSuccess)
                return fail(VX_EDEVICE, h2d_failed);
            if (ev && hipEventRecord(c->copy_ev[3 * timed + 1], st) == hipSuccess) {
                timed_bytes.push_back(sl.bytes);
                cp.copy_end = c->copy_ev[3 * timed + 1];  // doubles as the round's `copied` (copy stream)
                ev_k = (long)timed++;
            }
            return 0;
        };
    }
    // after cp.round: the kernel-end event; the round's timed-copy index or -1
    long kernel_end(int si, int rc) {
        if (!rc && ev_k >= 0 && hipEventRecord(c->copy_ev[3 * ev_k + 2], c->slots[si].stream) != hipSuccess)
            ev_k = -1;
        return ev_k;
    }
    // the round's timeline entry (t_submit / t_read_done: its reads queued / finished, ns)
    void push(uint64_t t_submit, uint64_t t_read_done, uint64_t bytes, uint64_t offset, uint32_t lanes,
              uint32_t flags) {
        vx_verify_round vr{};
        vr.read_submit_ms = rel_ms(t_submit);
        vr.read_done_ms = rel_ms(t_read_done);
        vr.enqueue_ms = rel_ms(t_enqueue);
        vr.bytes = bytes;
        vr.offset = offset;
        vr.lanes = lanes;
        vr.flags = flags;
        tl.push_back(vr);
        tl_ev.push_back(ev_k);
        t_last_enqueue = clk::now();
    }
    // after ChunkPipe::finish: the events into vx_verify_trace, the timeline to the context
    void fold(int rc) {
        vx_verify_trace& vt = c->last_verify;
        vt.tail_ms = std::chrono::duration<double, std::milli>(clk::now() - t_last_enqueue).count();
        if (!rc && timed) {  // finish() waited for every round: the copy events are complete
            float a = 0, b = 0, busy = 0;
            for (size_t k = 0; k < timed; ++k) {
                (void)hipEventElapsedTime(&a, c->copy_ev[0], c->copy_ev[3 * k]);
                (void)hipEventElapsedTime(&b, c->copy_ev[0], c->copy_ev[3 * k + 1]);
                busy += b - a;
                vt.copy_bytes += timed_bytes[k];
            }
            vt.copy_busy_ms = busy;
            vt.copy_span_ms = b;
            vt.rounds = (uint32_t)timed;
            // GPU times on the call's host clock, through the anchor
            const double base = anchored ? ((double)t_anchor - (double)c->verify_t0_ns) * 1e-6 : 0.0;
            for (size_t k = 0; k < tl.size() && anchored; ++k) {
                if (tl_ev[k] < 0) continue;
                float x = 0;
                const size_t e = 3 * (size_t)tl_ev[k];
                if (hipEventElapsedTime(&x, c->anchor_ev, c->copy_ev[e]) == hipSuccess) tl[k].copy_start_ms = base + x;
                if (hipEventElapsedTime(&x, c->anchor_ev, c->copy_ev[e + 1]) == hipSuccess) tl[k].copy_end_ms = base + x;
                if (hipEventElapsedTime(&x, c->anchor_ev, c->copy_ev[e + 2]) == hipSuccess) tl[k].kernel_end_ms = base + x;
            }
        }
        c->last_rounds = std::move(tl);
    }
};

}  // namespace vxe
