// vx_reverify.hip — bulk re-verify from disk (include/vx_hash.h, DESIGN.md
// §6.1/§6.3): vx_verify_files / _range / _multi and vx_last_verify*.
//
// Pieces shorter than two chunks (verify_chunk_for): the reader threads pread each slot's pieces
// straight into that slot's pinned stage (segments back to back,
// file_store.rs:240-298 byte ranges) and the slot launches while the next free
// slot is read.  Longer pieces: resumable chunked hashing — round k reads
// chunk k of every piece of a window into a slot, and the chunk kernel
// continues each piece's 20-byte SHA-1 state from round k-1, so PCIe moves
// round k+1 while the GPU compresses round k and no launch waits on a whole
// multi-MiB chain.  Completions are consumed here; they never reach vx_poll.
// With vx_set_skip_holes, pieces that lie wholly in ranges the file system
// never wrote are left out of both paths and judged against the SHA-1 of zeros
// (vx_extents.hpp).
#include "vx_chunk_pipe.hpp"

using namespace vxe;

namespace {

// Re-verify chunk size for `count` pieces: 256 KiB when
// every piece's chunk fits one slot arena (a single window of rounds), else
// 128 KiB.  A call split into windows ends on its last, smaller window, whose
// rounds are chain-bound; measured (profiles/r01/reverify/policy*.json):
// 1 MiB x 2,774 pieces 43.6 -> 46.8 GiB/s at 128 KiB, 256 KiB x 11,093 pieces
// 37.5 (whole-piece slots) -> 45.0, 2 MiB x 1,387 best at 256 KiB + ramp.
uint64_t verify_chunk_for(const vx_ctx* c, uint64_t count) {
    if (c->cfg.verify_chunk) return c->cfg.verify_chunk;
    constexpr uint64_t big = 256 * 1024, small = 128 * 1024;
    return count * big <= c->slots[0].arena_cap && count <= c->slots[0].cap ? big : small;
}

// Both verify the pieces `todo` (increasing; a sub-list of [first, first +
// count): the pieces a call over file holes still has to read, DESIGN.md §6.11,
// else all of them) of an n-piece torrent; tags, bad[] and matched_out are
// indexed from `first`.  Slot capacities and windows count pieces to do, so a
// sparse list does not make sparse slots or rounds.  Both queue reads up to
// kReadahead slots ahead of the slot being launched (see verify_chunked).
int verify_whole(FileVerify& fv, vx_files::Readers& rd, uint64_t n, uint32_t pl, uint64_t total, uint64_t first,
                 const std::vector<uint64_t>& todo) {
    vx_ctx* c = fv.c;
    const uint64_t stride = align_up(pl, kAlign);
    const uint64_t last_len = total - (n - 1) * (uint64_t)pl;
    const size_t nslots = c->slots.size();
    const size_t depth = nslots > 1 ? std::min<size_t>(kReadahead, nslots - 1) : 0;
    std::vector<std::vector<vx_files::ReadItem>> items(nslots);
    struct Queued {
        int si;
        uint64_t ticket;
    };
    std::deque<Queued> q;  // slots read or reading, in piece order, not yet launched
    // Runs of whole pieces inside one file go out as one pread of up to 4 MiB
    // (vx_files::Runs; 16 KiB pieces were pread-bound).
    vx_files::Runs runs = rd.runs(4ull << 20);
    // Ramps: nothing overlaps the first slot's read or the last slot's copy
    // and kernel, so the first slots take 1/2^L, ..., 1/4, 1/2 of a full
    // slot's pieces, the first one <= 64 MiB, and the last full slot's worth
    // is split in halves down to that size (cfg.verify_ramp = 0 turns both
    // off; as for chunks, §6.3).
    const uint64_t cap_full =
        std::min<uint64_t>(c->slots[0].cap, std::max<uint64_t>(1, c->slots[0].arena_cap / stride));
    int ramp = 0;
    while (c->cfg.verify_ramp > 0 && ramp < 8 && (cap_full >> ramp) > 1 && (cap_full >> ramp) * stride > (64ull << 20))
        ++ramp;
    int filled = 0;
    uint64_t next = 0;  // index into todo
    const uint64_t end = todo.size();
    int rc = 0;
    while ((next < end || !q.empty()) && !rc) {
        // The slot to launch next may wait for a free slot; later ones take
        // only a slot that is free now.
        while (next < end && q.size() <= depth) {
            int si = -1;
            rc = fv.slot(q.empty(), &si);
            if (rc || si < 0) break;
            Slot& s = c->slots[si];
            reset_fill(s);
            if ((rc = ensure_stage(c, s))) break;
            s.state = Slot::FILLING;  // reserved until launched
            s.t_open = std::chrono::steady_clock::now();
            uint64_t cap = filled < ramp ? std::max<uint64_t>(1, cap_full >> (ramp - filled)) : cap_full;
            const uint64_t rem = end - next, smallest = std::max<uint64_t>(1, cap_full >> ramp);
            if (ramp > 0 && rem <= cap && rem > smallest) cap = std::max(smallest, (rem + 1) / 2);
            ++filled;
            const uint64_t lo = next, hi = std::min<uint64_t>(end, next + cap);
            auto& it = items[si];
            it.clear();
            for (uint64_t t = lo; t < hi; ++t) {
                const uint64_t i = todo[t];
                const uint32_t len = (uint32_t)(i == n - 1 ? last_len : pl);
                const uint32_t k = (uint32_t)(t - lo);
                runs.add(it, s.stage.get() + k * stride, i, len);
                s.h_offsets[k] = k * stride;
                s.h_lens[k] = len;
                if (len != s.h_lens[0]) s.uniform = false;
                std::memcpy(s.h_expected + (size_t)k * 20, fv.expected + 20 * i, 20);
                s.tags.push_back(i - first);
            }
            s.n = (uint32_t)(hi - lo);
            s.has_expected = true;
            s.bytes = (hi - lo - 1) * stride + s.h_lens[s.n - 1];
            s.runs.push_back(Run{0, s.bytes});
            q.push_back(Queued{si, rd.submit(it)});
            next = hi;
        }
        if (rc || q.empty()) break;
        const Queued head = q.front();
        q.pop_front();
        rd.wait(head.ticket);
        rc = launch_slot(c, head.si);
        if (!rc) rc = reap(c, false);
        fv.consume();
    }
    rd.wait();  // error path: no read may still target a stage
    release_filling_slots(c);  // slots read but never launched (error path)
    return rc;
}

// The rounds of every window, in order, each read into its own slot by the
// reader pool and then enqueued (H2D + chunk kernel).  Reads run up to
// kReadahead rounds ahead of the round being enqueued (bounded by the slots),
// queued on the pool so the readers never wait for an enqueue: with one round
// of read-ahead the reads and the copy chain were coupled round by round, and
// every round whose read outlasted the previous copy left PCIe idle (the head
// ramp's doubling rounds most of all).  Each round's data
// copy is timed on the GPU (vx_tuning_last_verify).
int verify_chunked(FileVerify& fv, vx_files::Readers& rd, uint64_t n, uint32_t pl, uint64_t total, uint64_t first,
                   uint64_t cnt, const std::vector<uint64_t>& todo, const uint8_t* hole, uint64_t C) {
    vx_ctx* c = fv.c;
    const uint64_t last_len = total - (n - 1) * (uint64_t)pl;
    const uint64_t end = todo.size();  // windows and rounds index todo
    ChunkPipe cp(c);
    int rc = cp.open(cnt, fv.digests_out ? nullptr : fv.expected + 20 * first, "vx_verify_files");
    if (!rc && c->verify_copy_stream) rc = cp.use_copy_stream();
    cp.hole = hole;
    cp.bytes = end * (uint64_t)pl - (todo.back() == n - 1 ? (uint64_t)pl - last_len : 0);
    // windows of W pieces; each window runs its rounds in order
    const Slot& s0 = c->slots[0];
    const uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>(s0.cap, s0.arena_cap / C));
    struct Round {
        uint64_t w0, w1, a, len;
        bool continues;
        int si;
        uint32_t m;
        uint64_t ticket, bytes;
        uint32_t flags;          // VX_ROUND_* (the round timeline)
        uint64_t t_submit = 0;   // its reads queued (steady-clock ns)
    };
    std::vector<Round> rounds;
    for (uint64_t w0 = 0; w0 < end; w0 += W) {
        const uint64_t w1 = std::min<uint64_t>(end, w0 + W);
        const uint64_t wmax = todo[w1 - 1] == n - 1 ? std::max<uint64_t>(pl, last_len) : pl;
        const int ramp = (int)c->cfg.verify_ramp;
        const auto sched = chunk_schedule(wmax, C, w0 == 0 ? ramp : 0, w1 == end ? ramp : 0);
        for (size_t k = 0; k < sched.size(); ++k) {
            const uint64_t a = sched[k].first, len = sched[k].second;
            const uint32_t fl = (k == 0 ? VX_ROUND_NEW_WINDOW : 0u) |
                                (len < C && a < C && w0 == 0 ? VX_ROUND_HEAD_RAMP : 0u) |
                                (len < C && a >= C && w1 == end ? VX_ROUND_TAIL_RAMP : 0u);
            rounds.push_back(Round{w0, w1, a, len, k > 0, -1, 0, 0, 0, fl});
        }
    }
    const size_t nslots = c->slots.size();
    const size_t depth = nslots > 1 ? std::min<size_t>(kReadahead, nslots - 1) : 0;
    std::vector<std::vector<vx_files::ReadItem>> items(nslots);
    RoundTimeline tlm(c, cp, "vx_verify_files");
    auto consume = [&] { fv.consume(); };
    // Reserve a slot for round r and queue its reads; false when no slot is
    // free and `block` is not set.
    auto start_read = [&](Round& r, bool block) -> bool {
        int si = -1;
        rc = cp.slot(block, &si, consume);
        if (rc || si < 0) return false;
        Slot& s = c->slots[si];
        reset_fill(s);
        if ((rc = ensure_stage(c, s))) return false;
        // lanes 4 KiB apart: every stage destination can take an O_DIRECT read
        const uint64_t pitch = align_up(r.len, vx_files::DirectIo::kBlock);
        auto& it = items[si];
        it.clear();
        uint32_t m = 0;
        for (uint64_t t = r.w0; t < r.w1; ++t) {
            const uint64_t i = todo[t];
            const uint64_t len_i = i == n - 1 ? last_len : pl;
            if (r.a >= len_i && !(r.a == 0 && len_i == 0)) continue;  // piece already finished
            const uint64_t clen = std::min<uint64_t>(r.len, len_i - r.a);
            it.push_back(vx_files::ReadItem{s.stage.get() + (uint64_t)m * pitch, i, r.a, clen});
            s.h_offsets[m] = (uint64_t)m * pitch;
            s.h_lens[m] = (uint32_t)clen;
            s.h_pidx[m] = (uint32_t)(i - first);
            s.h_poff[m] = r.a;
            s.h_tlen[m] = len_i;
            ++m;
        }
        r.m = m;
        if (m == 0) return true;  // nothing to read or hash: the slot stays free
        s.state = Slot::FILLING;  // reserved until the round is enqueued
        s.bytes = r.bytes = (uint64_t)(m - 1) * pitch + s.h_lens[m - 1];
        r.si = si;
        r.t_submit = vx_files::Readers::now_ns();
        r.ticket = rd.submit(it);
        return true;
    };
    size_t nr = 0;  // next round to read
    for (size_t ne = 0; ne < rounds.size() && !rc; ++ne) {
        while (nr < rounds.size() && nr <= ne + depth && start_read(rounds[nr], nr == ne)) ++nr;
        if (rc) break;
        Round& r = rounds[ne];
        if (r.m == 0) continue;
        rd.wait(r.ticket);
        rc = cp.round(r.si, r.m, r.continues, false, tlm.timed_copy());
        tlm.kernel_end(r.si, rc);
        tlm.push(r.t_submit, rd.done_ns(r.ticket), r.bytes, r.a, r.m, r.flags);
    }
    rd.wait();  // error path: no read may still target a stage
    release_filling_slots(c);  // rounds read but never launched (error path)
    rc = cp.finish(fv.digests_out ? nullptr : fv.matched_out, fv.digests_out, rc, fv.bad.data());
    tlm.fold(rc);
    if (!rc && !fv.digests_out)
        for (uint64_t i = 0; i < cnt; ++i)
            if (fv.bad[i]) fv.matched_out[i] = 0;
    fv.done = cnt;
    return rc;
}

}  // namespace

namespace vxe {

int ensure_holes(vx_ctx* c, const char* who) {
    vx_ctx::Holes& h = c->holes;
    if (h.d) return 0;  // made together, this one last
    if (!h.stream && !h.stream.make(hipStreamNonBlocking))
        return fail(VX_EDEVICE, std::string(who) + ": stream creation failed");
    if ((!h.t0 && !h.t0.make(hipEventDefault)) || (!h.t1 && !h.t1.make(hipEventDefault)) ||  // (timed)
        !h.h.reserve(h.kZeroBlock) || !h.d.reserve(h.kZeroBlock))
        return fail(VX_ENOMEM, std::string(who) + ": zero-hash buffers");
    return 0;
}

vx_extents::Holes scan_holes(vx_ctx* c, const std::vector<int>& fds, const uint64_t* file_lengths) {
    c->holes.last = vx_hole_trace{};
    if (!c->holes.skip) return vx_extents::Holes();
    const uint64_t t0 = vx_files::Readers::now_ns();
    vx_extents::Holes holes(fds, file_lengths);
    c->holes.last.extents = holes.extents();
    c->holes.last.scan_ms = (vx_files::Readers::now_ns() - t0) * 1e-6;
    return holes;
}

// vx_verify_files_range, and with sp the engine's side of a split
// (vx_verify_files_split: pieces [sp->first, sp->end), always chunk rounds).
int64_t verify_files_impl(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                          uint32_t piece_length, const uint8_t* expected, size_t n_pieces, size_t first,
                          size_t count, uint8_t* matched_out, uint32_t io_threads, vx_split* sp,
                          uint8_t* digests_out) {
    // digests_out set: vx_hash_files.  No expected table, always chunk rounds
    // (ChunkPipe keeps the digests), matched_out is the call's ok_out (may be NULL).
    const bool hashing = digests_out != nullptr;
    if (!c || (nfiles && (!paths || !file_lengths)) || piece_length == 0 ||
        (!hashing && ((n_pieces && !expected) || (count && !matched_out))))
        return fail(VX_EINVAL, "vx_verify_files: bad argument");
    if (first > n_pieces || count > n_pieces - first)
        return fail(VX_EINVAL, "vx_verify_files: piece range outside the torrent");
    if (c->sticky) return c->sticky;
    if (c->pending || c->filling >= 0) return fail(VX_EBUSY, "vx_verify_files: async pieces pending");
    uint64_t total = 0;
    for (size_t f = 0; f < nfiles; ++f) total += file_lengths[f];
    if (n_pieces != (total + piece_length - 1) / piece_length)
        return fail(VX_EINVAL, "vx_verify_files: n_pieces does not match the files' total length");
    if (count == 0) return 0;
    const uint64_t C = verify_chunk_for(c, count);
    bool chunked = piece_length >= 2 * C || sp || hashing;  // the split and the hash call always stream chunk rounds
    if (piece_length > c->cfg.max_piece_len) chunked = true;  // whole pieces would not fit a slot
    if (chunked ? c->slots[0].arena_cap < std::min<uint64_t>(C, align_up(piece_length, vx_files::DirectIo::kBlock))
                : piece_length > c->cfg.max_piece_len)
        return fail(VX_ERANGE, "vx_verify_files: pieces do not fit the context's slots");
    int rc = set_device(c);
    if (rc) return rc;

    const uint64_t end = first + count;
    const uint64_t t_call = vx_files::Readers::now_ns();
    c->last_verify = vx_verify_trace{};
    c->last_rounds.clear();
    c->verify_t0_ns = t_call;
    const std::vector<vx_files::FileSpan> fs = vx_files::layout(file_lengths, nfiles, piece_length);
    std::vector<int> fds(nfiles, -1);
    for (size_t f = 0; f < nfiles; ++f) fds[f] = open(paths[f], O_RDONLY | O_CLOEXEC);
    const int nthreads = io_threads ? (int)io_threads : (int)std::max(1u, std::min(16u, usable_cpus()));
    std::vector<uint8_t> bad(count, 0);
    if (!sp && matched_out) std::memset(matched_out, 0, count);  // (the split's pool writes its entries concurrently)
    // Pieces that lie wholly in file holes are judged without a read (DESIGN.md
    // §6.11): todo keeps the others.  The split and the hash call do not ask.
    const uint64_t last_len = total - (n_pieces - 1) * (uint64_t)piece_length;
    c->holes.last = vx_hole_trace{};
    std::vector<uint64_t> todo;
    std::vector<uint8_t> is_hole;  // per piece of the range; empty: none is
    ZeroDigests zero(c, "vx_verify_files");
    if (!sp && !hashing) {
        const vx_extents::Holes holes = scan_holes(c, fds, file_lengths);
        if (holes.any()) {
            vx_hole_trace& ht = c->holes.last;
            const uint64_t t_class = vx_files::Readers::now_ns();
            std::vector<vx_files::Seg> segs;
            uint32_t lens[2];
            int nlens = 0;
            is_hole.assign(count, 0);
            for (uint64_t i = first; i < end; ++i) {
                if (!holes.hole_piece(fs, (int64_t)i, piece_length, segs)) continue;
                const uint32_t len = (uint32_t)(i == n_pieces - 1 ? last_len : piece_length);
                is_hole[i - first] = 1;
                ht.hole_pieces++;
                ht.hole_bytes += len;
                if (nlens < 2 && std::find(lens, lens + nlens, len) == lens + nlens) lens[nlens++] = len;
            }
            ht.scan_ms += (vx_files::Readers::now_ns() - t_class) * 1e-6;
            if (!ht.hole_pieces) is_hole.clear();
            else if ((rc = zero.start(lens, nlens))) is_hole.clear();  // (fails the call below: nothing was read yet)
        }
    }
    todo.reserve(count);
    for (uint64_t i = first; i < end && !rc; ++i)
        if (is_hole.empty() || !is_hole[i - first]) todo.push_back(i);
    {
        const vx_files::DirectIo dio(fds, c->cfg.direct_io != 0);
        vx_files::Readers rd(nthreads, fs, fds, piece_length, bad.data(), first, &dio);
        FileVerify fv{c, expected, matched_out, bad};
        fv.digests_out = digests_out;
        c->harvest_counts_mismatches = false;
        // Uncached data: the disk binds, and takes bigger reads better.
        const uint64_t Cc = c->cfg.verify_cold_chunk;
        const uint64_t Cv = chunked && !c->cfg.verify_chunk && c->cfg.direct_io && Cc > C &&
                                    piece_length >= 2 * Cc && c->slots[0].arena_cap >= Cc &&
                                    dio.resident_fraction() < 0.5
                                ? Cc
                                : C;
        c->last_verify.chunk_bytes = chunked ? Cv : 0;
        uint64_t lowest = end;
        const int regime = c->cfg.direct_io && dio.resident_fraction() < 0.5 ? 1 : 0;  // the split's learned figures
        if (rc || (!sp && todo.empty())) {
            // the zero hashes failed to start, or every piece is a hole: no round
        } else if (sp) {
            rc = verify_split(fv, rd, sp, n_pieces, piece_length, total, Cv, &lowest, regime);
        } else if (chunked) {
            rc = verify_chunked(fv, rd, n_pieces, piece_length, total, first, count, todo,
                                is_hole.empty() ? nullptr : is_hole.data(), Cv);
        } else {
            rc = verify_whole(fv, rd, n_pieces, piece_length, total, first, todo);
        }

        if (!rc && !chunked) {
            while (fv.done < todo.size() && !rc) {
                rc = reap(c, true);
                fv.consume();
                bool any = false;
                for (auto& s : c->slots) any |= s.state == Slot::INFLIGHT;
                if (!any && fv.done < todo.size() && !rc) rc = fail(VX_EDEVICE, "vx_verify_files: lost completions");
            }
        }
        c->harvest_counts_mismatches = true;
        trace_reads(c->last_verify, rd, dio, t_call);
        if (rc) {
            // The call fails and its results are dropped: wait for every slot
            // still reading the stages, then free them without harvest(), so
            // abandoned pieces never reach vx_stats.
            wait_and_free_inflight(c);
            c->done.clear();
        }
        for (size_t i = 0; i < count && hashing && !rc; ++i) {  // never a digest over bytes that were not read
            if (matched_out) matched_out[i] = !bad[i];
            if (bad[i]) std::memset(digests_out + i * 20, 0, 20);
        }
    }
    // The hole pieces' verdicts: the expected row against the zero digest of
    // the piece's length (started before the first read, waited for here; also
    // when the call failed, so nothing of it still runs).
    const int zrc = zero.wait();
    if (!rc) rc = zrc;
    for (uint64_t k = 0; k < is_hole.size() && !rc; ++k) {
        if (!is_hole[k]) continue;
        const uint64_t i = first + k;
        const uint32_t len = (uint32_t)(i == n_pieces - 1 ? last_len : piece_length);
        const uint8_t* z = zero.get(len);
        const bool ok = z && std::memcmp(expected + 20 * i, z, 20) == 0;
        matched_out[k] = ok ? 1 : 0;
        c->stats.pieces_completed++;
        c->stats.bytes_completed += len;
        c->stats.pieces_mismatched += !ok;
    }
    return end_files_call(c, fds, bad, t_call, rc);
}

int check_contexts(vx_ctx* const* ctxs, size_t nctx, const char* who) {
    for (size_t k = 0; k < nctx; ++k) {
        if (!ctxs[k]) return fail(VX_EINVAL, std::string(who) + ": NULL context");
        for (size_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return fail(VX_EINVAL, std::string(who) + ": a context appears twice");
    }
    return 0;
}

int64_t fan_out(size_t nctx, const std::function<int64_t(size_t)>& fn) {
    std::vector<int64_t> rcs(nctx, 0);
    std::vector<std::string> errs(nctx);
    auto run = [&](size_t k) {
        rcs[k] = fn(k);
        if (rcs[k] < 0) errs[k] = g_err;  // g_err is thread-local
    };
    std::vector<std::thread> th;
    th.reserve(nctx);
    size_t started = 1;
    try {
        for (; started < nctx; ++started) th.emplace_back(run, started);
    } catch (...) {  // could not start a thread: run the rest on this one
    }
    run(0);
    for (size_t k = started; k < nctx; ++k) run(k);
    for (auto& t : th) t.join();
    int64_t nbad = 0;
    for (size_t k = 0; k < nctx; ++k) {
        if (rcs[k] < 0) {
            g_err = "context " + std::to_string(k) + ": " + errs[k];
            return rcs[k];
        }
        nbad += rcs[k];
    }
    return nbad;
}

}  // namespace vxe

extern "C" {

int64_t vx_verify_files_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                              uint32_t piece_length, const uint8_t* expected, size_t n_pieces, size_t first,
                              size_t count, uint8_t* matched_out, uint32_t io_threads) {
    return verify_files_impl(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces, first, count,
                             matched_out, io_threads, nullptr);
}

int64_t vx_hash_files_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                            uint32_t piece_length, size_t n_pieces, size_t first, size_t count, uint8_t* digests_out,
                            uint8_t* ok_out, uint32_t io_threads) {
    // (what needs no context first, as the other hash calls)
    if (!c) return fail(VX_EINVAL, "vx_hash_files: NULL context");
    if ((nfiles && (!paths || !file_lengths)) || piece_length == 0 || !digests_out)
        return fail(VX_EINVAL, "vx_hash_files: NULL paths/file_lengths/digests_out, or piece_length 0");
    uint64_t total = 0;
    for (size_t f = 0; f < nfiles; ++f) total += file_lengths[f];
    if (n_pieces != (total + piece_length - 1) / piece_length)
        return fail(VX_EINVAL, "vx_hash_files: n_pieces does not match the files' total length");
    if (first > n_pieces || count > n_pieces - first)
        return fail(VX_EINVAL, "vx_hash_files: piece range outside the torrent");
    return verify_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, n_pieces, first, count, ok_out,
                             io_threads, nullptr, digests_out);
}

int64_t vx_hash_files(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                      uint32_t piece_length, size_t n_pieces, uint8_t* digests_out, uint8_t* ok_out,
                      uint32_t io_threads) {
    return vx_hash_files_range(c, paths, file_lengths, nfiles, piece_length, n_pieces, 0, n_pieces, digests_out, ok_out,
                               io_threads);
}

int64_t vx_verify_files(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                        uint32_t piece_length, const uint8_t* expected, size_t n_pieces, uint8_t* matched_out,
                        uint32_t io_threads) {
    return vx_verify_files_range(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces, 0, n_pieces,
                                 matched_out, io_threads);
}

// In-process multi-device re-verify: vortex is ONE process
// with one event loop (event_loop.rs:385), so where torch.distributed would
// run one process per GPU, a Rust caller holds one context per GPU and this
// call splits [0, n_pieces) across them by the same contiguous rule as
// vortex_amd.shard.shard_range (n/nctx each, remainder to the last
// contexts), one host thread per context.  Each thread runs
// vx_verify_files_range on its context and writes its slice of matched_out
// in place, so no merge step is needed.
int64_t vx_verify_files_multi(vx_ctx* const* ctxs, size_t nctx, const char* const* paths,
                              const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
                              const uint8_t* expected, size_t n_pieces, uint8_t* matched_out, uint32_t io_threads) {
    if (!ctxs || nctx == 0 || nctx > 1024) return fail(VX_EINVAL, "vx_verify_files_multi: bad context list");
    if (int rc = check_contexts(ctxs, nctx, "vx_verify_files_multi")) return rc;
    if (n_pieces && (!expected || !matched_out)) return fail(VX_EINVAL, "vx_verify_files_multi: bad argument");
    const uint32_t total_io = io_threads ? io_threads : std::max(1u, std::min(16u, usable_cpus()));
    const uint32_t per_ctx = std::max<uint32_t>(1, total_io / (uint32_t)nctx);
    const size_t base = n_pieces / nctx, rem = n_pieces % nctx, extra_from = nctx - rem;
    return fan_out(nctx, [&](size_t k) {
        const size_t first = k * base + (k > extra_from ? k - extra_from : 0);
        const size_t count = base + (k >= extra_from ? 1 : 0);
        return vx_verify_files_range(ctxs[k], paths, file_lengths, nfiles, piece_length, expected, n_pieces, first,
                                     count, matched_out + first, per_ctx);
    });
}

int vx_set_skip_holes(vx_ctx* c, int on) {
    if (!c || (on != 0 && on != 1)) return fail(VX_EINVAL, "vx_set_skip_holes: NULL context, or on not 0/1");
    c->holes.skip = on;
    return 0;
}

int vx_last_verify_holes(const vx_ctx* c, vx_hole_trace* out) {
    if (!c || !out) return fail(VX_EINVAL, "vx_last_verify_holes: NULL argument");
    *out = c->holes.last;
    return 0;
}

int vx_sha1_device_zeros(const uint32_t* d_lens, uint32_t n, void* d_digests, void* stream) {
    if (n == 0) return 0;
    if (!d_lens || !d_digests) return fail(VX_EINVAL, "vx_sha1_device_zeros: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_lens) | reinterpret_cast<uintptr_t>(d_digests)) & 3)
        return fail(VX_EINVAL, "vx_sha1_device_zeros: d_lens and d_digests must be 4-byte aligned");
    hipError_t e = vx::launch_sha1_zeros(d_lens, n, static_cast<uint8_t*>(d_digests), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "sha1 zero kernel launch");
}

int vx_last_verify(const vx_ctx* c, vx_verify_trace* out) {
    if (!c || !out) return fail(VX_EINVAL, "vx_last_verify: NULL argument");
    *out = c->last_verify;
    return 0;
}

int64_t vx_last_verify_rounds(const vx_ctx* c, vx_verify_round* out, size_t max) {
    if (!c || (max && !out)) return fail(VX_EINVAL, "vx_last_verify_rounds: NULL argument");
    const size_t k = std::min(max, c->last_rounds.size());
    if (k) std::memcpy(out, c->last_rounds.data(), k * sizeof(vx_verify_round));
    return (int64_t)c->last_rounds.size();
}

size_t vx_tuning_chunk_schedule(uint64_t L, uint64_t C, int head, int tail, uint64_t* out, size_t max) {
    if (C < 4 || C % 4) return 0;
    const auto r = chunk_schedule(L, C, std::max(0, std::min(5, head)), std::max(0, std::min(5, tail)));
    for (size_t i = 0; i < r.size() && i < max && out; ++i) {
        out[2 * i] = r[i].first;
        out[2 * i + 1] = r[i].second;
    }
    return r.size();
}

}  // extern "C"
