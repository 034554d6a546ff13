// vx_slots.hip — the download path of vx_hash.h:
// vx_submit / vx_merkle_submit / vx_hybrid_submit, vx_flush, the three polls
// and vx_drain.  A piece of any kind (v1: a SHA-1 digest; v2: a SHA-256 merkle
// root; hybrid: both from one transfer) is appended to the filling slot, and a
// slot holds one kind (Slot::Kind):
//  * submit_impl: guards, the open slot (fits), the kind's buffers, placement
//    (place), the kind's expected rows (record_rows), commit and launch;
//  * launch_slot_impl: one enqueue sequence per kind (launch_v1, launch_v2,
//    launch_hybrid) over the steps they share (copy_runs, gather_into_arena,
//    mark_inflight);
//  * harvest / reap / poll_impl: results back, per kind.
// The file re-verify (vx_reverify.hip) fills slots by hand and launches them
// as v1 slots through launch_slot; the chunk rounds (vx_chunk_pipe.hpp) use
// chain_h2d / mark_launched / reap.
#include "vx_engine_internal.hpp"

namespace vxe {

using Kind = Slot::Kind;

// zc_loader_wins: the slot size below which a batch is latency-bound
constexpr uint32_t kZcMinPieces = 128;

// The v2 buffers of slot s (vx_merkle_submit), allocated on its first v2 piece:
// a context that only sees v1 pieces allocates nothing for v2.
static int ensure_v2(Slot& s) {
    if (s.v2.d) return 0;  // (made last)
    const size_t bytes = (size_t)s.cap * (32 + 32 + 1) + 64;
    if (!s.v2.h.reserve(bytes) || !s.v2.d.reserve(bytes))
        return fail(VX_ENOMEM, "vx_merkle_submit: v2 metadata allocation failed");
    uint8_t *const h = s.v2.h_exp32 = s.v2.h.get(), *const d = s.v2.d_exp32 = s.v2.d.get();
    s.v2.h_roots = h + (size_t)s.cap * 32;
    s.v2.h_log2w = h + (size_t)s.cap * 64;
    s.v2.d_roots = d + (size_t)s.cap * 32;
    s.v2.d_log2w = d + (size_t)s.cap * 64;
    return 0;
}

// The hybrid buffers of slot s (vx_hybrid_submit), allocated on its first
// hybrid piece, beside the v2 block that takes the roots.
static int ensure_hybrid(Slot& s) {
    if (int rc = ensure_v2(s)) return rc;
    if (s.hy.joined) return 0;  // (made last)
    const size_t bytes = vx_hybrid_slot::pack(s.cap).bytes;
    if (!s.hy.h.reserve(bytes) || !s.hy.d.reserve(bytes) || !s.hy.joined.make(hipEventDisableTiming))
        return fail(VX_ENOMEM, "vx_hybrid_submit: hybrid metadata allocation failed");
    return 0;
}

// A host batch's unregistered pieces reach the pinned stage here, split by
// bytes over up to 16 threads: one thread's memcpy (~10-13 GiB/s) bounded
// config 3 from plain memory.  The caller's buffers stay
// valid because vx_*_batch returns only after every slot has completed (or,
// on an error, after every in-flight slot has been waited for: abandon_batch).
// A thread that cannot be created leaves its range to the calling thread, so
// no exception crosses the C ABI.
static void stage_copies(Slot& s) {
    if (s.staged.empty()) return;
    const uint64_t per = 16ull << 20;
    static const unsigned hw = usable_cpus();
    const unsigned T = (unsigned)std::min<uint64_t>({16, hw, std::max<uint64_t>(1, s.staged_bytes / per)});
    auto copy = [&s](size_t a, size_t b) {
        for (size_t k = a; k < b; ++k) std::memcpy(s.stage.get() + s.staged[k].off, s.staged[k].src, s.staged[k].len);
    };
    if (T <= 1) copy(0, s.staged.size());
    else {
        // contiguous ranges of roughly staged_bytes / T each
        std::vector<size_t> cut{0};
        uint64_t acc = 0, next = s.staged_bytes / T;
        for (size_t k = 0; k < s.staged.size() && cut.size() < T; ++k) {
            acc += s.staged[k].len;
            if (acc >= next) {
                cut.push_back(k + 1);
                next += s.staged_bytes / T;
            }
        }
        cut.push_back(s.staged.size());
        std::vector<std::thread> th;
        th.reserve(cut.size());
        size_t t = 1;
        try {
            for (; t + 1 < cut.size(); ++t) th.emplace_back(copy, cut[t], cut[t + 1]);
        } catch (...) {  // std::system_error (EAGAIN) or bad_alloc: copy the rest here
        }
        copy(cut[0], cut[1]);
        for (size_t u = t; u + 1 < cut.size(); ++u) copy(cut[u], cut[u + 1]);
        for (auto& x : th) x.join();
    }
    s.staged.clear();
    s.staged_bytes = 0;
}

// Order slot si's H2D after the previously launched slot's (one PCIe stream
// of copies across all slots): the host waits for the previous slot's copy,
// with no cross-stream wait.  That keeps copies back to back with a gap of
// one host wake-up and blocks the host for at most one batch's copy.  The
// alternatives measured worse and were removed in round 4 (EXPERIMENTS.md):
// a stream wait on the previous `copied` event blocked hipMemcpyAsync for
// ~8-9 ms at a time and left PCIe idle (34-46 GiB/s, 38-40 with an extra
// host wait two launches back), one dedicated copy stream 45, this 48.5-48.7
// (8192 x 256 KiB through vx_verify_batch, profiles/r01/h2d_modes/).
int chain_h2d(vx_ctx* c, int si) {
    const int last = c->last_launched;
    if (last >= 0 && last != si) VX_HIP(hipEventSynchronize(c->slots[last].copied));
    return 0;
}

void mark_launched(vx_ctx* c, int si) { c->last_launched = si; }

// Every eligible slot goes zero-copy: the kernel beats gather + hash
// everywhere measured (profiles/r03/zero_copy/).  Full async slots (round-3 A/B, alternating
// runs of async_probe, one registered mmap per buffer): 16 KiB 33 -> 48
// GiB/s, 256 / 512 KiB 47.8 -> 48.8 / 48.1 -> 49.0, 1 / 2 / 4 MiB 44 -> 48 /
// 34 -> 44 / 30 -> 35.  Small, latency-bound batches (round-3 loop-latency A/B,
// 32-piece batches) only in the three-wave form: download-loop p50 at 32 KiB
// 0.68 ms against 0.70, 256 KiB 3.75 against 3.75, 2 MiB 26.6 against 27.7.

// The loader wave takes the loads off the producer, so the chain reading host
// memory runs at 0.78 us per block instead of 0.83-0.86 (tools/zc_chain_probe
// .py): latency-bound batches then finish 7-9 % sooner (p50 at 256 KiB 3.75
// ms against 4.13, 2 MiB 26.7 against 28.8).  On full slots, where PCIe
// binds, it ran 2-4 % behind the pair (256 KiB streamed 49.1 against 50.9
// GiB/s; ab_loader3.jsonl), so those keep the pair.
bool zc_loader_wins(uint32_t n) { return n < kZcMinPieces; }

// ---- the launch: what the kinds share ----

// The slot's direct runs, then its staged runs, into the arena.
static int copy_runs(Slot& s, hipStream_t cs) {
    for (const DirectRun& r : s.druns)
        VX_HIP(hipMemcpyAsync(s.d_arena.get() + r.lo, r.host, r.hi - r.lo, hipMemcpyHostToDevice, cs));
    for (const Run& r : s.runs)
        VX_HIP(hipMemcpyAsync(s.d_arena.get() + r.lo, s.stage.get() + r.lo, r.hi - r.lo, hipMemcpyHostToDevice, cs));
    return 0;
}

// The gather kernel over the slot's registered pieces; the four tables are
// already on the device (a hybrid slot's lie in its packed block).
static int gather_into_arena(vx_ctx* c, Slot& s, const uint64_t* d_src, const uint64_t* d_offsets,
                             const uint32_t* d_lens, const uint32_t* d_tfirst, hipStream_t cs) {
    // Slots of long pieces (>= 2 MiB on average) hash with a few
    // chain-bound pairs that barely touch HBM, so the gather may use 128
    // workgroups: async 2 / 4 MiB pieces 39.8 -> 43.2 / 35.8 -> 39.6 GiB/s.
    // With shorter pieces the hash kernels compete and 128 cost up to 10 %
    // (1 MiB: -2 %).
    const uint32_t grid = s.bytes >= (uint64_t)s.n << 21 ? 128u : 0u;
    hipError_t e = vx::launch_gather(d_src, d_offsets, d_lens, d_tfirst, s.n, s.gtiles, s.d_arena.get(), cs, grid);
    if (e != hipSuccess) return hip_fail(e, "gather launch");
    c->stats.gather_tiles += s.gtiles;
    return 0;
}

// A v1 or v2 slot's pieces into its arena, data before metadata: the deferred
// stage copies, behind the copy chain the runs, and with `tables` the offsets
// and lengths and, over registered pieces, the gather behind its own tables.
static int copy_pieces(vx_ctx* c, int si, bool tables) {
    Slot& s = c->slots[si];
    hipStream_t cs = s.stream;
    stage_copies(s);
    if (int rc = chain_h2d(c, si)) return rc;
    if (int rc = copy_runs(s, cs)) return rc;
    if (!tables) return 0;
    VX_HIP(hipMemcpyAsync(s.d_offsets, s.h_offsets, (size_t)s.n * 8, hipMemcpyHostToDevice, cs));
    VX_HIP(hipMemcpyAsync(s.d_lens, s.h_lens, (size_t)s.n * 4, hipMemcpyHostToDevice, cs));
    if (!s.gtiles) return 0;
    VX_HIP(hipMemcpyAsync(s.d_src, s.h_src, (size_t)s.n * 8, hipMemcpyHostToDevice, cs));
    VX_HIP(hipMemcpyAsync(s.d_tfirst, s.h_tfirst, (size_t)(s.n + 1) * 4, hipMemcpyHostToDevice, cs));
    return gather_into_arena(c, s, s.d_src, s.d_offsets, s.d_lens, s.d_tfirst, cs);
}

// The end of every launch: the verdict column back, `done` behind it.
static int mark_inflight(vx_ctx* c, Slot& s) {
    if (s.has_expected) VX_HIP(hipMemcpyAsync(s.h_matched, s.d_matched, s.n, hipMemcpyDeviceToHost, s.stream));
    VX_HIP(hipEventRecord(s.done, s.stream));
    s.state = Slot::INFLIGHT;
    s.seq = c->seq++;
    c->stats.batches++;
    return 0;
}

// ---- the launch: one enqueue sequence per kind ----

// H2D(data) → H2D(meta) → `copied` → kernel → D2H(digests, verdicts).
static int launch_v1(vx_ctx* c, int si) {
    Slot& s = c->slots[si];
    hipStream_t cs = s.stream;
    const uint32_t n = s.n;
    // Zero-copy slot: every piece is read by the hash kernel itself, so no
    // bytes cross PCIe ahead of it and nothing waits for the copy chain.
    // Any slot qualifies, async or inside a host batch (vx_hash.h).  (all_mapped:
    // it has nothing staged and no runs.)
    const bool zc = s.gtiles && s.all_mapped && c->cfg.zero_copy;
    if (zc) {
        VX_HIP(hipMemcpyAsync(s.d_lens, s.h_lens, (size_t)n * 4, hipMemcpyHostToDevice, cs));
        VX_HIP(hipMemcpyAsync(s.d_src, s.h_src, (size_t)n * 8, hipMemcpyHostToDevice, cs));
    } else if (int rc = copy_pieces(c, si, !s.uniform || s.gtiles)) {  // (the uniform kernel reads no table)
        return rc;
    }
    if (s.use_table)
        VX_HIP(hipMemcpyAsync(s.d_pidx, s.h_pidx, (size_t)n * 4, hipMemcpyHostToDevice, cs));
    else if (s.has_expected)
        VX_HIP(hipMemcpyAsync(s.d_expected, s.h_expected, (size_t)n * 20, hipMemcpyHostToDevice, cs));
    const uint8_t* d_exp = s.use_table ? c->d_table.get() : (s.has_expected ? s.d_expected : nullptr);
    const uint32_t* d_row = s.use_table ? s.d_pidx : nullptr;
    VX_HIP(hipEventRecord(s.copied, cs));
    mark_launched(c, si);
    hipError_t e;
    if (zc) {
        const bool loader = zc_loader_wins(n);
        e = vx::launch_zero_copy(s.d_src, s.d_lens, n, s.d_digests, d_exp, s.d_matched, loader, cs, d_row);
        c->stats.zero_copy_slots++;
        c->stats.zero_copy_loader_slots += loader;
    } else if (s.uniform) {
        const uint32_t len = s.h_lens[0];
        const uint64_t stride = align_up(std::max<uint32_t>(len, 1), kAlign);
        e = vx::launch_uniform(s.d_arena.get(), stride, len, n, s.d_digests, d_exp, s.d_matched, cs, vx::kUniformDefault,
                               d_row);
    } else {
        uint64_t max_len = 0, total = 0;
        for (uint32_t i = 0; i < n; ++i) {
            max_len = std::max<uint64_t>(max_len, s.h_lens[i]);
            total += s.h_lens[i];
        }
        e = vx::launch_ragged(s.d_arena.get(), s.d_offsets, s.d_lens, nullptr, n, s.d_digests, d_exp, s.d_matched, cs,
                              vx::plan_ragged(n, max_len, total), d_row);
    }
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    VX_HIP(hipMemcpyAsync(s.h_digests, s.d_digests, (size_t)n * 20, hipMemcpyDeviceToHost, cs));
    return mark_inflight(c, s);
}

// As launch_v1, not zero-copy unless vx_set_merkle_zero_copy: a v2 slot has no
// chain for the transfer to hide behind, so gather-then-hash loses only the
// hash of one leaf.  The fused piece kernel runs at the
// slot's widest tree; above 256 leaves it leaves tile tops in d_tops and the
// node kernel follows (launch_merkle_pieces).  With the setting on, a slot
// that qualifies as a v1 slot does (every piece registered and 16-byte
// aligned: nothing staged, no runs) is hashed by the zero-copy piece kernel
// through the pieces' device mappings: only the lens, srcs, log2w and expected
// tables go ahead of it, and nothing waits for the copy chain.
static int launch_v2(vx_ctx* c, int si) {
    Slot& s = c->slots[si];
    Slot::V2& v = s.v2;
    hipStream_t cs = s.stream;
    const uint32_t n = s.n, K = v.kmax;
    const bool zc = c->merkle_zc && s.gtiles && s.all_mapped;
    if (zc) {
        VX_HIP(hipMemcpyAsync(s.d_lens, s.h_lens, (size_t)n * 4, hipMemcpyHostToDevice, cs));
        VX_HIP(hipMemcpyAsync(s.d_src, s.h_src, (size_t)n * 8, hipMemcpyHostToDevice, cs));
    } else if (int rc = copy_pieces(c, si, true)) {
        return rc;
    }
    VX_HIP(hipMemcpyAsync(v.d_log2w, v.h_log2w, n, hipMemcpyHostToDevice, cs));
    if (s.has_expected) VX_HIP(hipMemcpyAsync(v.d_exp32, v.h_exp32, (size_t)n * 32, hipMemcpyHostToDevice, cs));
    VX_HIP(hipEventRecord(s.copied, cs));
    mark_launched(c, si);
    uint8_t *d_exp = s.has_expected ? v.d_exp32 : nullptr, *d_matched = s.has_expected ? s.d_matched : nullptr;
    hipError_t e;
    if (zc) {
        if (!v.d_tops.reserve(vx::merkle_pieces_work(n, K))) return fail(VX_ENOMEM, "v2 tile tops allocation failed");
        e = vx::launch_merkle_zc_pieces(s.d_src, s.d_lens, v.d_log2w, n, K, v.d_tops.get(), v.d_roots, d_exp, d_matched,
                                        cs);
        // vx_get_stats is the same with the setting on or off: the slot's tiles cross PCIe once either
        // way and count as pulled from registered memory; which kernel pulled them is the trace's
        c->stats.gather_tiles += s.gtiles;
        c->merkle_zc_trace.slots++;
        c->merkle_zc_trace.pieces += n;
        for (uint32_t i = 0; i < n; ++i) c->merkle_zc_trace.bytes += s.h_lens[i];
    } else {
        c->merkle_zc_trace.fallback_slots += c->merkle_zc != 0;
#if VX_MERKLE_ASYNC_FUSED
        if (!v.d_tops.reserve(vx::merkle_pieces_work(n, K))) return fail(VX_ENOMEM, "v2 tile tops allocation failed");
        e = vx::launch_merkle_pieces(s.d_arena.get(), s.d_offsets, s.d_lens, v.d_log2w, n, K, v.d_tops.get(), v.d_roots,
                                     d_exp, d_matched, cs);
#else  // the A/B leg (vx_tuning.h): the leaf + node pair, d_tops its leaf array
        if (!v.d_tops.reserve(((uint64_t)n << K) * 32)) return fail(VX_ENOMEM, "v2 tile tops allocation failed");
        e = vx::launch_merkle_ragged(s.d_arena.get(), s.d_offsets, s.d_lens, v.d_log2w, n, K, v.d_tops.get(), v.d_roots,
                                     d_exp, d_matched, cs);
#endif
    }
    if (e != hipSuccess) return hip_fail(e, "merkle piece kernel launch");
    VX_HIP(hipMemcpyAsync(v.h_roots, v.d_roots, (size_t)n * 32, hipMemcpyDeviceToHost, cs));
    return mark_inflight(c, s);
}

// A hybrid slot.  Both hashes read the one copy in the arena,
// so the slot is never zero-copy:
//   1. one H2D of the whole metadata block, then the copies or the gather, on
//      the slot's stream; `copied`;
//   2. the context's side stream waits for `copied` and runs the merkle piece
//      path with no expected rows; `joined`;
//   3. the slot's stream hashes every piece's whole data blocks: an unpadded
//      piece's chunk is final and emits its digest, a padded one keeps its state;
//   4. the slot's stream waits for `joined` and runs the finish kernel;
//   5. D2H of digests, roots and verdicts; `done` (mark_inflight).
// So the merkle work hides beside the SHA-1 chain, as it does when the two
// submits of a piece land in two slots.
static int launch_hybrid(vx_ctx* c, int si) {
    Slot& s = c->slots[si];
    Slot::Hybrid& hy = s.hy;
    const uint32_t n = s.n, K = s.v2.kmax;
    hipStream_t cs = s.stream;
    if (!c->hy_stream) {
        // High priority, as the re-verify's copy stream (vx_chunk_pipe.hpp): HIP keeps a
        // priority's streams on hardware queues of their own.  At the default priority the
        // side stream shared a queue with one slot's stream, and every other slot's merkle
        // kernel (0.7 ms, and what its finish kernel waits for) queued behind that slot's
        // 3 ms chain (profiles/hybrid/async.json, "side_stream").
        int least = 0, greatest = 0;
        VX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        if (!c->hy_stream.make_with_priority(hipStreamNonBlocking, greatest))
            return fail(VX_EDEVICE, "hybrid launch: side stream creation failed");
    }
    if (!s.v2.d_tops.reserve(vx::merkle_pieces_work(n, K)))
        return fail(VX_ENOMEM, "hybrid tile tops allocation failed");
    // pack what the submits filled in (vx_hybrid_slot::Pack)
    const vx_hybrid_slot::Pack p = vx_hybrid_slot::pack(n);
    uint8_t *h = hy.h.get(), *d = hy.d.get();
    auto h64 = [&](size_t o) { return reinterpret_cast<uint64_t*>(h + o); };
    auto h32 = [&](size_t o) { return reinterpret_cast<uint32_t*>(h + o); };
    std::memcpy(h + p.offsets, s.h_offsets, (size_t)n * 8);
    std::memset(h + p.poffs, 0, (size_t)n * 8);
    std::memcpy(h + p.src, s.h_src, (size_t)n * 8);
    std::memcpy(h + p.lens, s.h_lens, (size_t)n * 4);
    std::memcpy(h + p.rows, s.h_pidx, (size_t)n * 4);
    std::memcpy(h + p.tfirst, s.h_tfirst, (size_t)(n + 1) * 4);
    for (uint32_t i = 0; i < n; ++i) {
        const Slot::Hybrid::Row& r = hy.rows[i];
        const vx_hybrid_slot::Lane& l = r.lane;
        h64(p.tail_offs)[i] = l.tail_off;
        h64(p.totals)[i] = l.total;
        h32(p.pads)[i] = l.pad;
        h32(p.chunks)[i] = l.chunk;
        h32(p.ident)[i] = i;
        std::memcpy(h + p.exp_sha1 + (size_t)i * 20, r.sha1, 20);
        std::memcpy(h + p.exp_roots + (size_t)i * 32, r.root, 32);
        h[p.flags + i] = l.flags;
        h[p.log2w + i] = r.log2w;
    }
    auto d64 = [&](size_t o) { return reinterpret_cast<uint64_t*>(d + o); };
    auto d32 = [&](size_t o) { return reinterpret_cast<uint32_t*>(d + o); };
    if (int rc = chain_h2d(c, si)) return rc;
    VX_HIP(hipMemcpyAsync(d, h, p.copy_bytes, hipMemcpyHostToDevice, cs));
    if (int rc = copy_runs(s, cs)) return rc;
    if (s.gtiles)
        if (int rc = gather_into_arena(c, s, d64(p.src), d64(p.offsets), d32(p.lens), d32(p.tfirst), cs)) return rc;
    VX_HIP(hipEventRecord(s.copied, cs));
    mark_launched(c, si);
    // the merkle side, beside the chain
    VX_HIP(hipStreamWaitEvent(c->hy_stream, s.copied, 0));
    hipError_t e = vx::launch_merkle_pieces(s.d_arena.get(), d64(p.offsets), d32(p.lens), d + p.log2w, n, K, s.v2.d_tops.get(),
                                            s.v2.d_roots, nullptr, nullptr, c->hy_stream);
    if (e != hipSuccess) return hip_fail(e, "hybrid merkle piece kernel launch");
    VX_HIP(hipEventRecord(hy.joined, c->hy_stream));
    // the SHA-1 side: whole data blocks, then the join and the finish kernel
    uint32_t* d_states = d32(p.states);
    e = vx::launch_chunk(s.d_arena.get(), d64(p.offsets), d32(p.chunks), n, d32(p.ident), d64(p.poffs), d64(p.totals),
                         d_states, s.d_digests, nullptr, nullptr, cs);
    if (e != hipSuccess) return hip_fail(e, "hybrid chunk kernel launch");
    VX_HIP(hipStreamWaitEvent(cs, hy.joined, 0));
    const uint8_t* exp1 = s.use_table ? c->d_hy_sha1.get() : d + p.exp_sha1;
    const uint8_t* exp2 = s.use_table ? c->d_hy_roots.get() : d + p.exp_roots;
    e = vx::launch_hybrid_finish(s.d_arena.get(), d64(p.tail_offs), d32(p.lens), d32(p.pads), n, hy.total ? hy.total : 64,
                                 d_states, s.d_digests, s.v2.d_roots, exp1, exp2, s.use_table ? d32(p.rows) : nullptr,
                                 d + p.flags, s.d_matched, cs);
    if (e != hipSuccess) return hip_fail(e, "hybrid finish kernel launch");
    VX_HIP(hipMemcpyAsync(s.h_digests, s.d_digests, (size_t)n * 20, hipMemcpyDeviceToHost, cs));
    VX_HIP(hipMemcpyAsync(s.v2.h_roots, s.v2.d_roots, (size_t)n * 32, hipMemcpyDeviceToHost, cs));
    return mark_inflight(c, s);  // (a hybrid slot always has_expected: which sides count is the lanes' flags)
}

static int launch_slot_impl(vx_ctx* c, int si) {
    Slot& s = c->slots[si];
    if (c->filling == si) {
        c->filling = -1;
        c->flush_pending = false;
    }
    if (s.n == 0) {
        s.state = Slot::FREE;
        return 0;
    }
    switch (s.kind) {
        case Kind::V2: return launch_v2(c, si);
        case Kind::Hybrid: return launch_hybrid(c, si);
        default: return launch_v1(c, si);
    }
}

// A failed launch leaves a slot half-enqueued: the context turns sticky and
// every later call reports the error (vx_destroy still cleans up).
int launch_slot(vx_ctx* c, int si) {
#ifdef VX_TEST_HOOKS
    if (c->fail_launch_after >= 0 && c->fail_launch_after-- == 0)
        return c->sticky = fail(VX_EDEVICE, "launch: injected device failure (vx_tuning_fail_launch_after)");
#endif
    const int rc = launch_slot_impl(c, si);
    if (rc) c->sticky = rc;
    return rc;
}

// ---- results ----

// Batch latency: first piece queued -> results harvested, into the log2
// histogram of vx_stats.
static void record_batch_latency(vx_ctx* c, std::chrono::steady_clock::time_point t_open) {
    const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_open);
    const uint64_t v = (uint64_t)std::max<int64_t>(0, us.count());
    vx_stats& st = c->stats;
    st.batch_latency_count++;
    st.batch_latency_sum_us += v;
    st.batch_latency_max_us = std::max(st.batch_latency_max_us, v);
    int k = 0;
    while (k + 1 < VX_STATS_HIST && (v >> (k + 1)) != 0) ++k;
    st.batch_latency_hist[k]++;
}

// A new completion at the back of its kind's queue.
template <class Completion>
static Completion& completion(std::deque<Completion>& done, uint64_t tag, uint8_t matched) {
    done.emplace_back();
    done.back().tag = tag;
    done.back().matched = matched;
    return done.back();
}

static void harvest(vx_ctx* c, Slot& s) {
    uint64_t bytes = 0, bad = 0;
    for (uint32_t i = 0; i < s.n; ++i) {
        const uint8_t matched = s.has_expected ? s.h_matched[i] : 0;
        switch (s.kind) {
            case Kind::V1:
                std::memcpy(completion(c->done, s.tags[i], matched).digest, s.h_digests + (size_t)i * 20, 20);
                bad += s.has_expected && !matched;
                break;
            case Kind::V2:
                std::memcpy(completion(c->done_v2, s.tags[i], matched).root, s.v2.h_roots + (size_t)i * 32, 32);
                bad += s.has_expected && !matched;
                break;
            case Kind::Hybrid: {
                vx_hybrid_completion& r = completion(c->done_hy, s.tags[i], matched);
                std::memcpy(r.sha1, s.h_digests + (size_t)i * 20, 20);
                std::memcpy(r.root, s.v2.h_roots + (size_t)i * 32, 32);
                bad += (s.hy.rows[i].lane.flags & ~matched) != 0;  // once, when any compared side fails
                break;
            }
        }
        bytes += s.h_lens[i];
    }
    if (s.n) {
        c->stats.pieces_completed += s.n;
        if (c->harvest_counts_mismatches) c->stats.pieces_mismatched += bad;
        c->stats.bytes_completed += bytes;
        record_batch_latency(c, s.t_open);
    }
    reset_fill(s);
    s.state = Slot::FREE;
}

// Harvest finished slots (oldest first).  block=true waits for the oldest.
int reap(vx_ctx* c, bool block_oldest) {
    std::vector<int> order;
    for (int i = 0; i < (int)c->slots.size(); ++i)
        if (c->slots[i].state == Slot::INFLIGHT) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return c->slots[a].seq < c->slots[b].seq; });
    bool first = true;
    for (int i : order) {
        Slot& s = c->slots[i];
        hipError_t q = (block_oldest && first) ? hipEventSynchronize(s.done) : hipEventQuery(s.done);
        first = false;
        if (q == hipSuccess) {
            harvest(c, s);
        } else if (q != hipErrorNotReady) {
            c->sticky = hip_fail(q, "batch failed on device");
            return c->sticky;
        }
    }
    return 0;
}

// A flush may launch now if, after it, a slot is still free to fill (with a
// single slot: if nothing is in flight).
static bool may_launch_now(const vx_ctx* c) {
    int inflight = 0;
    for (const Slot& s : c->slots) inflight += s.state == Slot::INFLIGHT;
    return inflight < std::max(1, (int)c->slots.size() - 1);
}

// vx_poll / vx_merkle_poll / vx_hybrid_poll: harvest what has finished (slots
// of any kind), then hand out the caller's kind from its own queue.
template <class Completion>
static int64_t poll_impl(vx_ctx* c, std::deque<Completion>& done, Completion* out, size_t max) {
    int rc = set_device(c);
    if (rc) return rc;
    if (c->sticky) {
        // Failed context: hand out every result the device did produce (batches
        // that finished, harvested now or earlier), then the error.  The tags
        // never returned are the pieces to re-hash elsewhere.
        const int sticky = c->sticky;
        (void)reap(c, false);
        c->sticky = sticky;
        if (done.empty()) return sticky;
    } else {
        rc = reap(c, false);
        if (rc) return rc;
        if (c->flush_pending && c->filling >= 0 && may_launch_now(c) && (rc = launch_slot(c, c->filling))) return rc;
    }
    size_t k = 0;
    while (k < max && !done.empty()) {
        out[k++] = done.front();
        done.pop_front();
    }
    c->pending -= k;
    return (int64_t)k;
}

// ---- the submit ----

// may_wait = false (an async submit with refuse_when_full): harvest what has
// finished without blocking, and if no slot is free then, VX_EBUSY.
static int acquire_filling(vx_ctx* c, bool may_wait) {
    if (c->filling >= 0) return c->filling;
    for (int attempt = 0;; ++attempt) {
        for (int i = 0; i < (int)c->slots.size(); ++i) {
            if (c->slots[i].state == Slot::FREE) {
                reset_fill(c->slots[i]);
                c->slots[i].state = Slot::FILLING;
                c->filling = i;
                return i;
            }
        }
        if (!may_wait) {
            if (attempt > 0) {
                c->stats.submits_refused++;
                return fail(VX_EBUSY, "vx_submit: every slot in flight (refuse_when_full)");
            }
            if (int rc = reap(c, /*block_oldest=*/false)) return rc;
            continue;
        }
        const auto t0 = std::chrono::steady_clock::now();
        int rc = reap(c, /*block_oldest=*/true);
        c->stats.submit_stall_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                                        std::chrono::steady_clock::now() - t0).count();
        if (rc) return rc;
    }
}

// May piece p join the open slot s at arena offset off?  A slot holds either
// table-indexed or explicit-row pieces, and one kind; a hybrid slot's padded
// pieces have one total length (the finish kernel's final block); the merkle
// piece kernel runs (pieces << widest log2w) lanes, a 32-bit count.
static bool fits(const Slot& s, const Piece& p, uint64_t off) {
    if (s.n == s.cap || off + p.len > s.arena_cap) return false;
    if (s.n == 0) return true;
    if (s.kind != p.kind || s.use_table != p.table) return false;
    if (p.kind == Kind::V1) return true;
    const uint64_t total = p.pad_len ? (uint64_t)p.len + p.pad_len : 0;
    if (total && s.hy.total && s.hy.total != total) return false;
    return ((uint64_t)(s.n + 1) << std::max(s.v2.kmax, p.log2w)) <= (1ull << 31);
}

// Where piece s.n's `len` bytes at `data` come from at launch, for arena offset
// off: registered and 16-byte aligned, the gather kernel pulls them; registered,
// a direct copy; anything else goes through the slot's pinned stage.
static int place(vx_ctx* c, Slot& s, const uint8_t* data, uint32_t len, uint64_t off) {
    const uint32_t i = s.n;
    const uint8_t* dev = nullptr;
    s.h_src[i] = 0;
    if (i == 0) s.t_open = std::chrono::steady_clock::now();
    if (len && (reinterpret_cast<uintptr_t>(data) & 15) == 0 && is_registered(c, data, len, &dev)) {
        // Registered, 16-byte aligned: the launch's gather kernel pulls it
        // through the range's device mapping.
        s.h_src[i] = reinterpret_cast<uint64_t>(dev);
        s.gtiles += vx::gather_tiles(len);
    } else if (len) {
        // all_mapped is cleared below, once the piece is certainly queued: a
        // refused piece (VX_ENOMEM from ensure_stage) must not take the rest
        // of the slot off the zero-copy path.
        if (is_registered(c, data, len)) {
            // Pinned source: DMA straight from the caller's buffer at launch;
            // pieces adjacent in host memory AND in the arena share one copy.
            if (!s.druns.empty() && s.druns.back().hi == off &&
                s.druns.back().host + (s.druns.back().hi - s.druns.back().lo) == data)
                s.druns.back().hi = off + len;
            else
                s.druns.push_back(DirectRun{data, off, off + len});
        } else {
            if (int rc = ensure_stage(c, s)) return rc;
            c->stats.staged_bytes += len;
            if (c->bulk) {  // a host batch: copied in parallel at launch (stage_copies)
                s.staged.push_back(StageCopy{data, off, len});
                s.staged_bytes += len;
            } else {
                std::memcpy(s.stage.get() + off, data, len);
            }
            if (!s.runs.empty() && align_up(s.runs.back().hi, kAlign) == off)
                s.runs.back().hi = off + len;  // (off is aligned) the alignment gap travels too
            else
                s.runs.push_back(Run{off, off + len});
        }
        s.all_mapped = false;
    }
    s.h_offsets[i] = off;
    s.h_lens[i] = len;
    s.h_tfirst[i + 1] = s.gtiles;
    // Equal lengths at 256-byte aligned back-to-back offsets are a uniform
    // batch: offset(i) = i * align_up(len, 256) (the uniform kernel's layout).
    if (i > 0 && len != s.h_lens[0]) s.uniform = false;
    return 0;
}

// Piece s.n's explicit expected row (v1: 20 bytes, v2: 32) into the slot's rows.
static void record_explicit_row(Slot& s, uint8_t* h_exp, size_t dlen, const uint8_t* expected) {
    const uint32_t i = s.n;
    if (expected) {
        std::memcpy(h_exp + (size_t)i * dlen, expected, dlen);
        // earlier pieces of this batch had no expected row: they get
        // matched = 0 against a zero row, which nobody reads.
        if (i > 0 && !s.has_expected) std::memset(h_exp, 0, (size_t)i * dlen);
        s.has_expected = true;
    } else if (s.has_expected) {
        std::memset(h_exp + (size_t)i * dlen, 0, dlen);
    }
}

// What piece s.n's kind keeps for the launch beside its placement.
static void record_rows(Slot& s, const Piece& p, uint64_t off) {
    const uint32_t i = s.n;
    s.kind = p.kind;
    switch (p.kind) {
        case Kind::V1:
            if (p.table)
                s.h_pidx[i] = p.row;
            else
                record_explicit_row(s, s.h_expected, VX_DIGEST_LEN, p.expected);
            s.use_table = p.table;
            s.has_expected |= p.table;
            break;
        case Kind::V2:
            s.v2.h_log2w[i] = (uint8_t)p.log2w;
            s.v2.kmax = std::max(s.v2.kmax, p.log2w);
            record_explicit_row(s, s.v2.h_exp32, VX_SHA256_LEN, p.expected);
            break;
        case Kind::Hybrid: {
            // The verdict column always comes back; which sides were given is the
            // lane's flags, so a side's bit is exact and not "compared with a zero row".
            const uint8_t flags = p.table ? 3 : (uint8_t)((p.expected ? 1 : 0) | (p.exp_root ? 2 : 0));
            Slot::Hybrid::Row row{vx_hybrid_slot::lane(off, p.len, p.pad_len, flags), {}, {}, (uint8_t)p.log2w};
            if (p.expected) std::memcpy(row.sha1, p.expected, VX_DIGEST_LEN);
            if (p.exp_root) std::memcpy(row.root, p.exp_root, VX_SHA256_LEN);
            s.hy.rows.push_back(row);
            s.v2.kmax = std::max(s.v2.kmax, p.log2w);
            if (p.pad_len) s.hy.total = (uint64_t)p.len + p.pad_len;
            s.h_pidx[i] = p.table ? p.row : i;
            s.use_table = p.table;
            s.has_expected = true;
            break;
        }
    }
}

// The last committed piece leaves the slot again (the launch it triggered failed).
static void uncommit(vx_ctx* c, Slot& s) {
    s.tags.pop_back();
    if (s.kind == Kind::Hybrid) s.hy.rows.pop_back();
    s.n--;
    c->pending--;
}

int submit_impl(vx_ctx* c, const Piece& p) {
    // 1. guards
    if (c->sticky) return c->sticky;
    if (!p.data && p.len) return fail(VX_EINVAL, "vx_submit: data is NULL");
    if (p.len > c->cfg.max_piece_len) return fail(VX_ERANGE, "vx_submit: piece longer than max_piece_len");
#ifdef VX_TEST_HOOKS
    if (c->fail_submit_after >= 0 && c->fail_submit_after-- == 0)
        return fail(VX_ENOMEM, "vx_submit: injected failure (vx_tuning_fail_submit_after)");
#endif
    // 2. the open slot, launched first if the piece does not fit it
    const bool may_wait = !c->cfg.refuse_when_full || c->bulk;  // host batches always wait
    int si = acquire_filling(c, may_wait);
    if (si < 0) return si;
    Slot* s = &c->slots[si];
    uint64_t off = align_up(s->bytes, kAlign);
    if (!fits(*s, p, off)) {
        if (int rc = launch_slot(c, si)) return rc;
        si = acquire_filling(c, may_wait);
        if (si < 0) return si;
        s = &c->slots[si];
        off = 0;
    }
    // 3. the kind's buffers, 4. placement, 5. the kind's rows
    int rc = p.kind == Kind::V2 ? ensure_v2(*s) : p.kind == Kind::Hybrid ? ensure_hybrid(*s) : 0;
    if (!rc) rc = place(c, *s, p.data, p.len, off);
    if (rc) return rc;
    record_rows(*s, p, off);
    // 6. commit, and launch a full slot
    s->tags.push_back(p.tag);
    s->n++;
    s->bytes = off + std::max<uint32_t>(p.len, 1);
    c->pending++;
    if (s->n >= c->cfg.batch_pieces && !c->bulk) {
        if ((rc = launch_slot(c, si))) {
            // One rule for every submit (vx_hash.h): a non-zero return means
            // the piece was NOT taken.  The launch failed (the context is now
            // sticky), so this piece leaves the batch again and goes back to
            // the caller with the error; the rest of the slot stays pending and
            // is what the caller recovers after vx_poll reports the failure.
            uncommit(c, *s);
            return rc;
        }
    }
    return 0;
}

// The argument check of the v2 and hybrid submits (vx_hybrid_slot::check), then the piece.
static int checked_submit(vx_ctx* c, const char* who, const Piece& p) {
    const char* why = nullptr;
    if (int rc = vx_hybrid_slot::check(p.len, p.pad_len, p.log2w, c->cfg.max_piece_len, &why))
        return fail(rc, std::string(who) + ": " + why);
    if (int rc = set_device(c)) return rc;
    return submit_impl(c, p);
}

}  // namespace vxe

using namespace vxe;

extern "C" {

int vx_submit(vx_ctx* c, uint64_t tag, const uint8_t* data, uint32_t len, const uint8_t* expected) {
    if (!c) return fail(VX_EINVAL, "vx_submit: NULL context");
    if (int rc = set_device(c)) return rc;
    return submit_impl(c, {.kind = Kind::V1, .tag = tag, .data = data, .len = len, .expected = expected});
}

int vx_set_piece_table(vx_ctx* c, const uint8_t* table, uint32_t n_pieces) {
    if (!c || (n_pieces && !table)) return fail(VX_EINVAL, "vx_set_piece_table: bad argument");
    if (c->pending || c->filling >= 0) return fail(VX_EBUSY, "vx_set_piece_table: pieces in flight");
    if (int rc = set_device(c)) return rc;
    c->d_table.reset();
    c->n_table = 0;
    if (!n_pieces) return 0;
    if (!c->d_table.reserve((size_t)n_pieces * 20))
        return fail(VX_ENOMEM, "vx_set_piece_table: device allocation failed");
    VX_HIP(hipMemcpy(c->d_table.get(), table, (size_t)n_pieces * 20, hipMemcpyHostToDevice));
    c->n_table = n_pieces;
    return 0;
}

int vx_submit_piece(vx_ctx* c, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t piece_index) {
    if (!c) return fail(VX_EINVAL, "vx_submit_piece: NULL context");
    if (piece_index >= c->n_table) return fail(VX_EINVAL, "vx_submit_piece: piece_index outside the piece table");
    if (int rc = set_device(c)) return rc;
    return submit_impl(c, {.kind = Kind::V1, .tag = tag, .data = data, .len = len, .table = true, .row = piece_index});
}

// Launch the filling slot unless that would leave no slot free for the next
// submit: then the slot stays open and keeps collecting pieces, and vx_poll
// launches it as soon as a batch completes.  So under load batches grow
// instead of the event-loop thread blocking in vx_submit for a whole batch
// (DESIGN.md §6.5).
int vx_flush(vx_ctx* c) {
    if (!c) return fail(VX_EINVAL, "vx_flush: NULL context");
    if (c->sticky) return c->sticky;
    if (c->filling < 0 || c->slots[c->filling].n == 0) return 0;
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = reap(c, false))) return rc;
    if (!may_launch_now(c)) {
        c->flush_pending = true;
        return 0;
    }
    return launch_slot(c, c->filling);
}

int64_t vx_poll(vx_ctx* c, vx_completion* out, size_t max) {
    if (!c || (!out && max)) return fail(VX_EINVAL, "vx_poll: bad argument");
    return poll_impl(c, c->done, out, max);
}

int64_t vx_merkle_poll(vx_ctx* c, vx_merkle_completion* out, size_t max) {
    if (!c || (!out && max)) return fail(VX_EINVAL, "vx_merkle_poll: bad argument");
    return poll_impl(c, c->done_v2, out, max);
}

int64_t vx_hybrid_poll(vx_ctx* c, vx_hybrid_completion* out, size_t max) {
    if (!c || (!out && max)) return fail(VX_EINVAL, "vx_hybrid_poll: bad argument");
    return poll_impl(c, c->done_hy, out, max);
}

int vx_merkle_submit(vx_ctx* c, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t log2w,
                     const uint8_t* expected) {
    if (!c) return fail(VX_EINVAL, "vx_merkle_submit: NULL context");
    return checked_submit(c, "vx_merkle_submit",
                          {.kind = Kind::V2, .tag = tag, .data = data, .len = len, .expected = expected, .log2w = log2w});
}

int vx_set_merkle_zero_copy(vx_ctx* c, int on) {
    if (!c || (on != 0 && on != 1)) return fail(VX_EINVAL, "vx_set_merkle_zero_copy: NULL context, or on not 0/1");
    c->merkle_zc = on;
    return 0;
}

int vx_merkle_zero_copy_trace(const vx_ctx* c, vx_merkle_zc_trace* out) {
    if (!c || !out) return fail(VX_EINVAL, "vx_merkle_zero_copy_trace: NULL argument");
    *out = c->merkle_zc_trace;
    return 0;
}

int vx_hybrid_submit(vx_ctx* c, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t pad_len, uint32_t log2w,
                     const uint8_t* exp_sha1, const uint8_t* exp_root) {
    if (!c) return fail(VX_EINVAL, "vx_hybrid_submit: NULL context");
    return checked_submit(c, "vx_hybrid_submit", {.kind = Kind::Hybrid, .tag = tag, .data = data, .len = len,
                                                  .expected = exp_sha1, .exp_root = exp_root, .log2w = log2w,
                                                  .pad_len = pad_len});
}

int vx_hybrid_submit_piece(vx_ctx* c, uint64_t tag, const uint8_t* data, uint32_t len, uint32_t pad_len,
                           uint32_t log2w, uint32_t piece_index) {
    if (!c) return fail(VX_EINVAL, "vx_hybrid_submit_piece: NULL context");
    if (piece_index >= c->n_hy_table)
        return fail(VX_EINVAL, "vx_hybrid_submit_piece: piece_index outside the hybrid piece tables");
    return checked_submit(c, "vx_hybrid_submit_piece", {.kind = Kind::Hybrid, .tag = tag, .data = data, .len = len,
                                                        .table = true, .row = piece_index, .log2w = log2w,
                                                        .pad_len = pad_len});
}

int vx_hybrid_set_piece_tables(vx_ctx* c, const uint8_t* sha1_table, const uint8_t* roots_table, uint32_t n_pieces) {
    if (!c || (n_pieces && (!sha1_table || !roots_table)))
        return fail(VX_EINVAL, "vx_hybrid_set_piece_tables: bad argument");
    if (c->pending || c->filling >= 0) return fail(VX_EBUSY, "vx_hybrid_set_piece_tables: pieces in flight");
    if (int rc = set_device(c)) return rc;
    c->d_hy_sha1.reset();
    c->d_hy_roots.reset();
    c->n_hy_table = 0;
    if (!n_pieces) return 0;
    if (!c->d_hy_sha1.reserve((size_t)n_pieces * 20) || !c->d_hy_roots.reserve((size_t)n_pieces * 32))
        return fail(VX_ENOMEM, "vx_hybrid_set_piece_tables: device allocation failed");
    VX_HIP(hipMemcpy(c->d_hy_sha1.get(), sha1_table, (size_t)n_pieces * 20, hipMemcpyHostToDevice));
    VX_HIP(hipMemcpy(c->d_hy_roots.get(), roots_table, (size_t)n_pieces * 32, hipMemcpyHostToDevice));
    c->n_hy_table = n_pieces;
    return 0;
}

int vx_drain(vx_ctx* c, uint32_t timeout_ms) {
    if (!c) return fail(VX_EINVAL, "vx_drain: NULL context");
    if (c->sticky) return c->sticky;
    int rc = set_device(c);
    if (rc) return rc;
    if (c->filling >= 0 && (rc = launch_slot(c, c->filling))) return rc;  // forced, unlike vx_flush
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        bool any = false;
        for (auto& s : c->slots) any |= s.state == Slot::INFLIGHT;
        if (!any) return 0;
        if (timeout_ms == 0) {
            rc = reap(c, true);
        } else {
            rc = reap(c, false);
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms))
                return fail(VX_EBUSY, "vx_drain: timeout");
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        if (rc) return rc;
    }
}

uint64_t vx_pending(const vx_ctx* c) { return c ? c->pending : 0; }

}  // extern "C"
