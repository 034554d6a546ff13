// vx_hybrid.hip — the hybrid (BEP 52 "upgrade path", v1 + v2) entries of
// vx_hash.h: vx_hybrid_device_pieces and vx_hybrid_verify_files / _range
// (kernels in sha1_kernels.hip, sha1_tail_kernels.hip and sha256_kernels.hip;
// the rounds in vx_hybrid_rounds.hpp, run by vx_block_rounds.hpp), and the four tuning
// kernel entries.  The hybrid download path (vx_hybrid_submit) is in vx_slots.hip.
#include "vx_chunk_pipe.hpp"
#include "vx_hybrid_rounds.hpp"

using namespace vxe;

namespace {

// What one files call owns on the device and in pinned memory; gone when it
// returns (a re-verify is once per torrent; the slots and stages stay with the
// context).
struct HybridBufs {
    DeviceMem d;
    std::vector<PinnedMem> h_tab;
    std::vector<DeviceMem> d_tab;
    Event chain;
    // The zero-tail kernel runs beside the rounds on a stream of its own (a
    // 4 MiB pad is a 65,535-block chain that nothing but the verdict waits for):
    // per slot, `state` after the round's SHA-1 kernel and `tailed` after its tails.
    std::vector<Event> state, tailed;
    // The zero-run kernel of a round (file holes) runs beside
    // that round's SHA-1 kernel on a stream of its own, made when a call first
    // has a zero run: per slot, `tabled` after the round's tables are on the
    // device and `zeroed` after its zero runs.
    std::vector<Event> tabled, zeroed;
    // The two streams last: each is waited for and destroyed before the events
    // and the blocks above go.
    Stream tail_stream, run_stream;
    int make(uint64_t device_bytes, size_t nslots, uint64_t tab_bytes, const std::string& who) {
        h_tab.resize(nslots);
        d_tab.resize(nslots);
        if (!d.reserve(device_bytes)) return fail(VX_ENOMEM, who + ": buffer allocation failed");
        for (size_t k = 0; k < nslots; ++k)
            if (!h_tab[k].reserve(tab_bytes) || !d_tab[k].reserve(tab_bytes))
                return fail(VX_ENOMEM, who + ": buffer allocation failed");
        state.resize(nslots);
        tailed.resize(nslots);
        // (lowest priority: the tails yield to the rounds, and HIP keeps a
        // priority's streams on hardware queues of their own, so no round's
        // kernel queues behind a long tail)
        int least = 0, greatest = 0;
        bool ok = chain.make(hipEventDisableTiming) &&
                  hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
                  tail_stream.make_with_priority(hipStreamNonBlocking, least);
        for (size_t k = 0; k < nslots && ok; ++k)
            ok = state[k].make(hipEventDisableTiming) && tailed[k].make(hipEventDisableTiming);
        if (!ok) return fail(VX_EDEVICE, who + ": stream or event creation failed");
        return 0;
    }
    int make_run_stream(const std::string& who) {
        if (run_stream) return 0;
        tabled.resize(state.size());
        zeroed.resize(state.size());
        bool ok = run_stream.make(hipStreamNonBlocking);
        for (size_t k = 0; k < state.size() && ok; ++k)
            ok = tabled[k].make(hipEventDisableTiming) && zeroed[k].make(hipEventDisableTiming);
        if (!ok) return fail(VX_EDEVICE, who + ": stream or event creation failed");
        return 0;
    }
};

// sha1_out and rows_out set: the hash call (vx_hybrid_hash_files).  Both
// expected tables are absent; the kernels write digests and rows where the
// verify call keeps the expected ones, matched_out is the call's ok_out (may be
// NULL), and with tree_out the files' trees are built from the rows after the
// last round.
int64_t hybrid_files_impl(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                          uint32_t piece_length, const uint8_t* exp_sha1, const uint8_t* exp_roots, size_t n_pieces,
                          size_t first, size_t count, uint8_t* matched_out, uint32_t io_threads,
                          uint8_t* sha1_out = nullptr, uint8_t* rows_out = nullptr, uint8_t* tree_out = nullptr,
                          uint64_t tree_rows = 0) {
    const bool hashing = sha1_out && rows_out;
    const std::string who = hashing ? "vx_hybrid_hash_files" : "vx_hybrid_verify_files";
    const bool null_args = !paths || !file_lengths || (!hashing && (!exp_sha1 || !exp_roots || !matched_out));
    int rc = begin_block_call(c, who, null_args, "paths/file_lengths/exp_sha1/exp_roots/matched_out", file_lengths,
                              nfiles, piece_length, n_pieces, first, count, UINT32_MAX, tree_out, tree_rows);
    if (rc || count == 0) return rc;
    // A round is PCIe-bound when its copy outlasts its chain: at 0.76 us per
    // block and 50 GiB/s that takes ~640 lanes, so a round holds 1,024 chunks
    // where the arena allows, and 64 MiB at least.
    const uint64_t arena = c->slots[0].arena_cap / VX_MERKLE_BLOCK * VX_MERKLE_BLOCK;
    const uint64_t C = vx_hybrid::chunk_for(piece_length, arena);
    if (C == 0) return fail(VX_ERANGE, who + ": a slot holds no 16 KiB block");
    const uint64_t stage = std::min<uint64_t>(arena, std::max<uint64_t>(64ull << 20, 1024 * C));
    if ((rc = set_device(c))) return rc;

    // Chunks that lie wholly in file holes are not read: the
    // planner gives them no stage bytes, carries the SHA-1 state across them
    // with zero-run lanes and the tail lanes, and has their leaf rows written by
    // the zero-leaf kernel.  The files are opened now, for the scan; the hash
    // call does not ask.
    BlockCall call{c, who, first, count};
    if (!hashing && c->holes.skip) call.open_files(paths, nfiles);
    c->holes.last = vx_hole_trace{};
    const vx_extents::Holes holes = hashing ? vx_extents::Holes() : scan_holes(c, call.fds, file_lengths);
    vx_merkle::HolePredicate in_hole;
    if (holes.any())
        in_hole = [&holes](uint32_t f, uint64_t off, uint32_t len) { return holes.hole(f, (int64_t)off, len); };
    // What the rounds need at most (a dry run of the planner: no I/O): the
    // leaf rows of the largest window and the bytes of the largest table; and
    // the pieces with no byte to read, which the host judges after the rounds.
    uint64_t rows = 1, tab_bytes = 16;
    bool zero_runs = false;
    std::vector<uint32_t> hole_pid, hole_len;
    {
        vx_hybrid::Rounds dry(file_lengths, nfiles, piece_length, n_pieces, first, count, stage, C,
                              vx_hybrid::kRowBudget, vx_hybrid::kMaxRun, in_hole);
        vx_hybrid::Round r;
        while (dry.next(r)) {
            rows = std::max<uint64_t>(rows, (uint64_t)r.w_n << r.w_log2);
            tab_bytes = std::max<uint64_t>(tab_bytes, r.l_len.size() * 32 + r.t_len.size() * 20 + r.rows.size() * 8 +
                                                          r.z_pid.size() * 12);
            zero_runs |= !r.z_pid.empty();
            hole_pid.insert(hole_pid.end(), r.hole_pid.begin(), r.hole_pid.end());
            hole_len.insert(hole_len.end(), r.hole_len.begin(), r.hole_len.end());
        }
    }
    // per piece: state (20) | expected SHA-1 (20) | expected root (32) | v1 verdict | v2 verdict | log2w
    const uint64_t o_exp1 = count * 20, o_exp2 = align_up(o_exp1 + count * 20, 16), o_v1 = o_exp2 + count * 32;
    const uint64_t o_v2 = o_v1 + count, o_lw = o_v2 + count, o_leaves = align_up(o_lw + count, 16);
    // Data copies on the context's copy stream, kernels on the slot streams, as
    // the v1 chunk rounds: no copy waits behind a kernel.
    ChunkPipe pipe(c);
    if (c->verify_copy_stream && (rc = pipe.use_copy_stream())) return rc;
    HybridBufs hb;
    if ((rc = hb.make(o_leaves + rows * 32, c->slots.size(), tab_bytes, who))) return rc;
    uint32_t* d_states = hb.d.as<uint32_t>();
    uint8_t *const hbd = hb.d.get(), *d_exp1 = hbd + o_exp1, *d_exp2 = hbd + o_exp2, *d_v1 = hbd + o_v1, *d_v2 = hbd + o_v2;
    uint8_t *d_lw = hbd + o_lw, *d_leaves = hbd + o_leaves;

    if (zero_runs && (rc = hb.make_run_stream(who))) return rc;
    const bool up = hashing ||
                    (hipMemcpy(d_exp1, exp_sha1 + 20 * first, count * 20, hipMemcpyHostToDevice) == hipSuccess &&
                     hipMemcpy(d_exp2, exp_roots + 32 * first, count * 32, hipMemcpyHostToDevice) == hipSuccess);
    if ((rc = call.begin(up, paths, file_lengths, nfiles, piece_length, d_lw, d_v1, 2 * count, matched_out))) return rc;
    // The zero hashes: the full block's leaf row first (it is synchronous), then
    // the digests of the hole pieces' lengths, beside the rounds.
    ZeroDigests zero(c, who.c_str());
    if (in_hole) {
        uint32_t zlens[2];
        int nz = 0;
        for (uint32_t len : hole_len)
            if (nz < 2 && std::find(zlens, zlens + nz, len) == zlens + nz) zlens[nz++] = len;
        if ((rc = zero_leaf_row(c, who.c_str())) || (rc = zero.start(zlens, nz))) return call.end(rc, 0);
    }
    // hashing: the digests and rows land where the verify call keeps the expected ones
    uint8_t* const d_dig = hashing ? d_exp1 : nullptr;
    uint8_t* const d_rows = hashing ? d_exp2 : nullptr;
    const uint8_t* const k_exp1 = hashing ? nullptr : d_exp1;
    const uint8_t* const k_exp2 = hashing ? nullptr : d_exp2;
    uint8_t* const k_v1 = hashing ? nullptr : d_v1;
    uint8_t* const k_v2 = hashing ? nullptr : d_v2;
    // One round, its data already in slot si's stage.
    auto enqueue = [&](size_t si, const vx_hybrid::Round& r) -> int {
        Slot& s = c->slots[si];
        // the round's tables in one copy: the uint64 columns, then the uint32 ones
        const size_t m = r.l_len.size(), t = r.t_len.size(), z = r.z_pid.size();
        const size_t e = r.rows.size() - r.hole_blocks;  // the block kernel's entries; the hole blocks' follow
        uint8_t* h = hb.h_tab[si].get();
        size_t at = 0;
        auto put = [&](const void* src, size_t bytes) {
            std::memcpy(h + at, src, bytes);
            const size_t was = at;
            at += bytes;
            return was;
        };
        const size_t a_loff = put(r.l_off.data(), m * 8), a_lpoff = put(r.l_poff.data(), m * 8);
        const size_t a_ltlen = put(r.l_tlen.data(), m * 8), a_toff = put(r.t_off.data(), t * 8);
        const size_t a_llen = put(r.l_len.data(), m * 4), a_lpid = put(r.l_pid.data(), m * 4);
        const size_t a_tlen = put(r.t_len.data(), t * 4), a_tpad = put(r.t_pad.data(), t * 4);
        const size_t a_tpid = put(r.t_pid.data(), t * 4), a_rows = put(r.rows.data(), r.rows.size() * 4);
        const size_t a_lens = put(r.lens.data(), r.lens.size() * 4), a_zpid = put(r.z_pid.data(), z * 4);
        const size_t a_zpoff = put(r.z_poff.data(), z * 4), a_zblocks = put(r.z_blocks.data(), z * 4);
        uint8_t* d = hb.d_tab[si].get();
        auto u64 = [&](size_t o) { return reinterpret_cast<const uint64_t*>(d + o); };
        auto u32 = [&](size_t o) { return reinterpret_cast<const uint32_t*>(d + o); };
        hipStream_t cs = pipe.cs ? pipe.cs : s.stream;
        hipError_t err = hipSuccess;
        if (r.bytes) err = hipMemcpyAsync(s.d_arena.get(), s.stage.get(), r.bytes, hipMemcpyHostToDevice, cs);
        if (err == hipSuccess && pipe.cs) err = hipEventRecord(s.copied, cs);
        if (err == hipSuccess) err = hipMemcpyAsync(d, h, at, hipMemcpyHostToDevice, s.stream);
        if (err == hipSuccess && z) err = hipEventRecord(hb.tabled[si], s.stream);
        if (err == hipSuccess && pipe.cs) err = hipStreamWaitEvent(s.stream, s.copied, 0);
        if (err == hipSuccess && call.totals.rounds) err = hipStreamWaitEvent(s.stream, hb.chain, 0);
        if (const int injected = err == hipSuccess ? injected_launch_failure(c, who) : 0) return injected;
        if (err == hipSuccess && z) {
            // The zero runs: after the tables and the previous round's kernels,
            // beside this round's SHA-1 kernel (other state rows), which a chunk
            // of zero blocks would otherwise follow for as long as it takes itself.
            err = hipStreamWaitEvent(hb.run_stream, hb.tabled[si], 0);
            if (err == hipSuccess && call.totals.rounds) err = hipStreamWaitEvent(hb.run_stream, hb.chain, 0);
            if (err == hipSuccess)
                err = vx::launch_zero_run(u32(a_zpid), u32(a_zpoff), u32(a_zblocks), (uint32_t)z, d_states,
                                          hb.run_stream);
            if (err == hipSuccess) err = hipEventRecord(hb.zeroed[si], hb.run_stream);
        }
        if (err == hipSuccess)
            err = vx::launch_chunk(s.d_arena.get(), u64(a_loff), u32(a_llen), (uint32_t)m, u32(a_lpid), u64(a_lpoff),
                                   u64(a_ltlen), d_states, d_dig, k_exp1, k_v1, s.stream);
        if (err == hipSuccess && t) {  // the tails: after the states, beside everything else
            err = hipEventRecord(hb.state[si], s.stream);
            if (err == hipSuccess) err = hipStreamWaitEvent(hb.tail_stream, hb.state[si], 0);
            if (err == hipSuccess)
                err = vx::launch_zero_tail(s.d_arena.get(), u64(a_toff), u32(a_tlen), u32(a_tpad), u32(a_tpid), (uint32_t)t,
                                           piece_length, d_states, d_dig, k_exp1, k_v1, hb.tail_stream);
            if (err == hipSuccess) err = hipEventRecord(hb.tailed[si], hb.tail_stream);
        }
        if (err == hipSuccess && e)
            err = vx::launch_merkle_blocks(s.d_arena.get(), u32(a_rows), u32(a_lens), (uint32_t)e, d_leaves, s.stream);
        if (err == hipSuccess && r.hole_blocks)
            err = vx::launch_merkle_zero_leaves(u32(a_rows) + e, u32(a_lens) + e, r.hole_blocks, d_leaves,
                                                c->holes.zero_leaf, s.stream);
        if (err == hipSuccess && r.end_window) {
            const uint64_t k = r.w_first - first;
            err = vx::launch_merkle_nodes(d_leaves, d_lw + k, r.w_n, r.w_log2, hashing ? d_rows + k * 32 : nullptr,
                                          hashing ? nullptr : k_exp2 + k * 32, hashing ? nullptr : k_v2 + k, s.stream);
        }
        if (err == hipSuccess && z) err = hipStreamWaitEvent(s.stream, hb.zeroed[si], 0);
        if (err == hipSuccess) err = hipEventRecord(hb.chain, s.stream);
        // the slot's arena and tables are free again once its tails have read them too
        if (err == hipSuccess && t) err = hipStreamWaitEvent(s.stream, hb.tailed[si], 0);
        if (err == hipSuccess) err = hipEventRecord(s.done, s.stream);
        if (err != hipSuccess) return hip_fail(err, (who + ": enqueue").c_str());
        c->stats.chunk_rounds++;
        c->holes.last.hole_pieces += r.hole_pid.size();
        c->holes.last.hole_blocks += r.hole_blocks;
        c->holes.last.hole_bytes += r.hole_bytes;
        return 0;
    };
    vx_files::Readers& rd = call.readers(io_threads, piece_length);
    vx_hybrid::Rounds plan(file_lengths, nfiles, piece_length, n_pieces, first, count, stage, C, vx_hybrid::kRowBudget,
                           vx_hybrid::kMaxRun, in_hole);
    rc = vx_block_rounds::run<vx_hybrid::Round>(plan, rd, c->slots.size(), call, enqueue, call.totals);
    if (pipe.cs && hipStreamSynchronize(pipe.cs) != hipSuccess && !rc)  // no copy may still read a stage
        rc = fail(VX_EDEVICE, who + ": a copy failed on the device");
    call.sync_slots(rc);
    if (hipStreamSynchronize(hb.tail_stream) != hipSuccess && !rc)
        rc = fail(VX_EDEVICE, who + ": a tail kernel failed on the device");
    if (hb.run_stream && hipStreamSynchronize(hb.run_stream) != hipSuccess && !rc)
        rc = fail(VX_EDEVICE, who + ": a zero-run kernel failed on the device");
    // (also when the call failed, so nothing of it still runs)
    if (const int zrc = zero.wait(); zrc && !rc) rc = zrc;
    std::vector<uint8_t> verdict(hashing ? 0 : 2 * count);
    if (!rc && !hashing && hipMemcpy(verdict.data(), d_v1, 2 * count, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(VX_EDEVICE, who + ": verdict download failed");
    // The pieces with no byte read: their v1 verdict is the expected row against
    // the zero digest of the piece's whole length; their root came from the node kernels.
    for (size_t k = 0; k < hole_pid.size() && !rc; ++k) {
        const uint8_t* zd = zero.get(hole_len[k]);
        verdict[hole_pid[k]] = zd && std::memcmp(exp_sha1 + 20 * (first + hole_pid[k]), zd, 20) == 0;
    }
    if (!rc && hashing &&
        (hipMemcpy(sha1_out, d_dig, count * 20, hipMemcpyDeviceToHost) != hipSuccess ||
         hipMemcpy(rows_out, d_rows, count * 32, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(VX_EDEVICE, who + ": digest and row download failed");
    if (!rc && tree_out)  // (the whole torrent: first == 0, count == n_pieces)
        rc = file_trees(c, d_rows, file_lengths, nfiles, piece_length, call.bad, tree_out, c->slots[0].stream, who);
    call.trace(C);
    int64_t n_failed = 0;
    uint64_t mism = 0;
    for (size_t i = 0; i < count && hashing && !rc; ++i) {  // never a digest or row over bytes that were not read
        if (matched_out) matched_out[i] = !call.bad[i];
        if (call.bad[i]) std::memset(sha1_out + i * 20, 0, 20), std::memset(rows_out + i * 32, 0, 32);
    }
    for (size_t i = 0; i < count && !hashing && !rc; ++i) {
        const uint8_t v = call.bad[i] ? 0 : (uint8_t)((verdict[i] ? 1 : 0) | (verdict[count + i] ? 2 : 0));
        matched_out[i] = v;
        n_failed += v != 3;
        mism += v != 3 && !call.bad[i];  // I/O errors count in io_errors only
    }
    const int64_t ended = call.end(rc, mism);
    return ended < 0 || hashing ? ended : n_failed;
}

}  // namespace

extern "C" {

int vx_hybrid_device_pieces(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint32_t* d_pads, const uint8_t* d_log2w, uint32_t n, uint32_t log2_width,
                            void* d_work, void* d_sha1, void* d_roots, const void* d_exp_sha1,
                            const void* d_exp_roots, void* d_matched, void* stream) {
    const char* who = "vx_hybrid_device_pieces";
    if (log2_width > VX_MERKLE_MAX_LOG2_WIDTH)
        return fail(VX_EINVAL, std::string(who) + ": log2_width > 17 (piece_length is 16384 << log2_width)");
    if (!d_base || !d_offsets || !d_lens || !d_pads || !d_work)
        return fail(VX_EINVAL, std::string(who) + ": NULL d_base, d_offsets, d_lens, d_pads or d_work");
    if ((d_exp_sha1 || d_exp_roots) && !d_matched)
        return fail(VX_EINVAL, std::string(who) + ": expected rows without d_matched");
    if ((reinterpret_cast<uintptr_t>(d_base) | reinterpret_cast<uintptr_t>(d_work) |
         reinterpret_cast<uintptr_t>(d_roots)) & 15)
        return fail(VX_EINVAL, std::string(who) + ": d_base, d_work and d_roots must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_sha1) | reinterpret_cast<uintptr_t>(d_exp_sha1) |
         reinterpret_cast<uintptr_t>(d_exp_roots)) & 3)
        return fail(VX_EINVAL, std::string(who) + ": d_sha1 and the expected rows must be 4-byte aligned");
    if (((uint64_t)n << log2_width) >> 32)
        return fail(VX_EINVAL, std::string(who) + ": n << log2_width does not fit 32 bits");
    if (n == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* w = static_cast<uint8_t*>(d_work);
    // d_work (vx_hash.h): the merkle piece kernel's work, then per piece 24
    // bytes of uint64 tables, 28 of uint32 and 2 verdicts
    uint8_t* tab = w + align_up(vx::merkle_pieces_work(n, log2_width), 16);
    uint64_t* tail_offs = reinterpret_cast<uint64_t*>(tab);
    uint64_t* poffs = tail_offs + n;
    uint64_t* tlens = poffs + n;
    uint32_t* clens = reinterpret_cast<uint32_t*>(tlens + n);
    uint32_t* pids = clens + n;
    uint32_t* states = pids + n;
    uint8_t* v1 = reinterpret_cast<uint8_t*>(states + (size_t)5 * n);
    uint8_t* v2 = v1 + n;
    const uint8_t* exp1 = static_cast<const uint8_t*>(d_exp_sha1);
    const uint8_t* exp2 = static_cast<const uint8_t*>(d_exp_roots);
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    hipError_t e = vx::launch_hybrid_prep(d_offsets, d_lens, d_pads, n, tail_offs, poffs, tlens, clens, pids, st);
    if (e == hipSuccess)
        e = vx::launch_chunk(base, d_offsets, clens, n, pids, poffs, tlens, states, static_cast<uint8_t*>(d_sha1),
                             exp1, exp1 ? v1 : nullptr, st);
    if (e == hipSuccess)
        e = vx::launch_zero_tail(base, tail_offs, d_lens, d_pads, nullptr, n, (uint64_t)VX_MERKLE_BLOCK << log2_width,
                                 states, static_cast<uint8_t*>(d_sha1), exp1, exp1 ? v1 : nullptr, st);
    if (e == hipSuccess)
        e = vx::launch_merkle_pieces(base, d_offsets, d_lens, d_log2w, n, log2_width, w,
                                     static_cast<uint8_t*>(d_roots), exp2, exp2 ? v2 : nullptr, st);
    if (e == hipSuccess && (exp1 || exp2))
        e = vx::launch_hybrid_merge(exp1 ? v1 : nullptr, exp2 ? v2 : nullptr, n, static_cast<uint8_t*>(d_matched),
                                    st);
    if (e != hipSuccess) return hip_fail(e, "hybrid piece kernels launch");
    return 0;
}

int vx_tuning_zero_tail_kernel(const void* d_base, const uint64_t* d_tail_offs, const uint32_t* d_lens,
                               const uint32_t* d_pads, uint32_t n, uint64_t piece_length, const uint32_t* d_states,
                               void* d_digests, void* stream) {
    if (n && (!d_base || !d_tail_offs || !d_lens || !d_pads || !d_states || !d_digests))
        return fail(VX_EINVAL, "vx_tuning_zero_tail_kernel: NULL argument");
    if (piece_length == 0 || (piece_length & 63))
        return fail(VX_EINVAL, "vx_tuning_zero_tail_kernel: piece_length must be a multiple of 64");
    hipError_t e = vx::launch_zero_tail(static_cast<const uint8_t*>(d_base), d_tail_offs, d_lens, d_pads, nullptr, n,
                                        piece_length, d_states, static_cast<uint8_t*>(d_digests), nullptr, nullptr,
                                        static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_zero_tail_kernel");
}

int vx_tuning_zero_run_kernel(const uint32_t* d_pids, const uint32_t* d_poffs, const uint32_t* d_blocks, uint32_t n,
                              uint32_t* d_states, void* stream) {
    if (n && (!d_pids || !d_poffs || !d_blocks || !d_states))
        return fail(VX_EINVAL, "vx_tuning_zero_run_kernel: NULL argument");
    hipError_t e = vx::launch_zero_run(d_pids, d_poffs, d_blocks, n, d_states, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_zero_run_kernel");
}

int vx_tuning_chunk_kernel(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t n,
                           const uint32_t* d_pids, const uint64_t* d_poffs, const uint64_t* d_tlens,
                           uint32_t* d_states, void* d_digests, void* stream) {
    if (n && (!d_base || !d_offsets || !d_lens || !d_pids || !d_poffs || !d_tlens || !d_states || !d_digests))
        return fail(VX_EINVAL, "vx_tuning_chunk_kernel: NULL argument");
    hipError_t e = vx::launch_chunk(static_cast<const uint8_t*>(d_base), d_offsets, d_lens, n, d_pids, d_poffs, d_tlens,
                                    d_states, static_cast<uint8_t*>(d_digests), nullptr, nullptr,
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_chunk_kernel");
}

int vx_tuning_hybrid_finish_kernel(const void* d_base, const uint64_t* d_tail_offs, const uint32_t* d_lens,
                                   const uint32_t* d_pads, uint32_t n, uint64_t padded_total,
                                   const uint32_t* d_states, void* d_digests, const void* d_roots,
                                   const void* d_exp_sha1, const void* d_exp_roots, const uint32_t* d_exp_index,
                                   const uint8_t* d_flags, void* d_matched, void* stream) {
    if (n && (!d_base || !d_tail_offs || !d_lens || !d_pads || !d_states || !d_digests || !d_roots || !d_exp_sha1 ||
              !d_exp_roots || !d_flags || !d_matched))
        return fail(VX_EINVAL, "vx_tuning_hybrid_finish_kernel: NULL argument");
    if (padded_total == 0 || (padded_total & 63))
        return fail(VX_EINVAL, "vx_tuning_hybrid_finish_kernel: padded_total must be a multiple of 64");
    hipError_t e = vx::launch_hybrid_finish(static_cast<const uint8_t*>(d_base), d_tail_offs, d_lens, d_pads, n,
                                            padded_total, d_states, static_cast<uint8_t*>(d_digests),
                                            static_cast<const uint8_t*>(d_roots),
                                            static_cast<const uint8_t*>(d_exp_sha1),
                                            static_cast<const uint8_t*>(d_exp_roots), d_exp_index, d_flags,
                                            static_cast<uint8_t*>(d_matched), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_hybrid_finish_kernel");
}

int64_t vx_hybrid_hash_files_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                                   uint32_t piece_length, size_t n_pieces, size_t first, size_t count,
                                   uint8_t* sha1_out, uint8_t* rows_out, uint8_t* ok_out, uint32_t io_threads) {
    if (!sha1_out || !rows_out) return fail(VX_EINVAL, "vx_hybrid_hash_files: NULL sha1_out or rows_out");
    return hybrid_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, nullptr, n_pieces, first, count,
                             ok_out, io_threads, sha1_out, rows_out);
}

int64_t vx_hybrid_hash_files(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                             uint32_t piece_length, size_t n_pieces, uint8_t* sha1_out, uint8_t* rows_out,
                             uint8_t* ok_out, uint8_t* tree_out, uint64_t tree_rows, uint32_t io_threads) {
    if (!sha1_out || !rows_out) return fail(VX_EINVAL, "vx_hybrid_hash_files: NULL sha1_out or rows_out");
    return hybrid_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, nullptr, n_pieces, 0, n_pieces,
                             ok_out, io_threads, sha1_out, rows_out, tree_out, tree_rows);
}

int64_t vx_hybrid_verify_files_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                                     uint32_t piece_length, const uint8_t* exp_sha1, const uint8_t* exp_roots,
                                     size_t n_pieces, size_t first, size_t count, uint8_t* matched_out,
                                     uint32_t io_threads) {
    return hybrid_files_impl(c, paths, file_lengths, nfiles, piece_length, exp_sha1, exp_roots, n_pieces, first, count,
                             matched_out, io_threads);
}

int64_t vx_hybrid_verify_files(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                               uint32_t piece_length, const uint8_t* exp_sha1, const uint8_t* exp_roots,
                               size_t n_pieces, uint8_t* matched_out, uint32_t io_threads) {
    return hybrid_files_impl(c, paths, file_lengths, nfiles, piece_length, exp_sha1, exp_roots, n_pieces, 0, n_pieces,
                             matched_out, io_threads);
}

}  // extern "C"
