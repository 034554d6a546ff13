// vx_split.hip — the self-balancing split (vx_verify_files_split, DESIGN.md
// §6.6): the claim word (vx_split_*), the engine's side of a split call
// (SplitRun), the cost model (vx_plan_verify*) and the split's tuning entries.
#include "vx_chunk_pipe.hpp"

using namespace vxe;

namespace {

// The claim word: head (low 32 bits) | stop (high 32).  The pool moves head
// up one piece per compare-and-swap (vx_split_claim); the engine moves stop
// down by a group (split_take_tail).  Neither side can take a piece the other
// has, and a group the engine asks for is cut to what is still unclaimed.
// The claimed pieces are [returned, *was) (*was: the stop before the claim).
// expect: the stop this engine left (UINT64_MAX: any); a different stop means
// an engine the split was not declared for (vx_split.engines) claims from it,
// and the call returns UINT64_MAX.
uint64_t split_take_tail(vx_split* s, uint64_t k, uint64_t expect = UINT64_MAX, uint64_t* was = nullptr) {
    uint64_t w = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    for (;;) {
        const uint64_t head = w & 0xffffffffull, stop = w >> 32;
        if (was) *was = stop;
        if (expect != UINT64_MAX && stop != expect) return UINT64_MAX;
        const uint64_t take = std::min(k, stop > head ? stop - head : 0);
        if (take == 0) return stop;
        const uint64_t nw = head | ((stop - take) << 32);
        if (__atomic_compare_exchange_n(&s->word, &w, nw, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE))
            return stop - take;
    }
}

// Streaming chunk rounds over pieces the engine claims from the top of the
// split as it goes.  A claimed piece takes a lane from its first chunk to its
// last, one C-byte chunk per round; every round carries all active lanes and
// the group that joins it (batch_chunked_gather's streaming rounds, here with
// the group sized at run time).  Before forming a round the engine estimates
//   T_engine(j) = the rounds its lanes (and j new pieces) still need, each
//                 max(bytes / intake, longest chunk's chain), plus the first
//                 round's read and the last kernel's chain
//   T_pool(j)   = (unclaimed - engines x j + half the pool's pieces in hand)
//                 / the pool's pace
// and takes the largest j with T_engine(j) <= T_pool(j).  The rates are
// measured in this call — the intake from the GPU copy events (first copy
// start to last copy end), the chain per 64-byte block from the kernel
// events, the pool's pace over its last 4 ms of vx_split_done — except for
// the first group, which starts from earlier split calls on this context (or
// the caller's per-thread rate, the PCIe rate and kChainBlock); its T_engine
// adds the lag earlier calls' single groups ended behind their prediction
// (the readers' start-up and the kernels trailing the copies).  No later
// group is formed until both sides have rates, and one only if it rides the
// active lanes' rounds and shortens the predicted end by a tenth — except
// for pieces of one chunk, whose groups cost one round each: those keep the
// first group's rule until the rates are in, and then only the model's.  Alone on
// the split (engines 1) the engine's pieces are the contiguous tail
// [*lowest, end); beside other engines, the groups it took.
// One call's state: the first nine members are verify_split's arguments, the
// rest set themselves up in declaration order; run() is the driver.
struct SplitRun {
    FileVerify& fv;
    vx_files::Readers& rd;
    vx_split* const sp;
    const uint64_t n;
    const uint32_t pl;
    const uint64_t total, C;
    uint64_t* const lowest;
    const int regime;

    vx_ctx* c = fv.c;
    const uint64_t first = sp->first, end = sp->end, cnt = end - first;
    const uint64_t last_len = total - (n - 1) * (uint64_t)pl;
    uint64_t plen(uint64_t i) const { return i == n - 1 ? last_len : (uint64_t)pl; }
    ChunkPipe cp{c};
    int open_pipe() {
        c->last_split.clear();
        int r = cp.open(cnt, fv.expected + 20 * first, "vx_verify_files_split");
        if (!r && c->verify_copy_stream) r = cp.use_copy_stream();
        return r;
    }
    int rc = open_pipe();
    const uint64_t longest = std::max<uint64_t>(pl, last_len);
    const uint64_t pitch = align_up(std::min<uint64_t>(C, longest), vx_files::DirectIo::kBlock);
    const Slot& s0 = c->slots[0];
    uint64_t max_lanes = std::max<uint64_t>(1, std::min<uint64_t>(s0.cap, s0.arena_cap / pitch));

    struct Lane {
        uint64_t piece, a;
        bool ramp;  // joined in the first round: chunks C/4, C/4, C/2, then C
    };
    std::vector<Lane> act;  // claimed pieces with chunks left, in join order
    // verify_chunked's ramps (chunk_schedule, depth 1), per lane.  Head: the
    // first group's first round is a C/4 chain and a quarter of the bytes, so
    // the call's first read and the copy that nothing overlaps are short
    // (later groups join rounds whose chain is C anyway).  Tail, every lane:
    // its last C bytes go as C/2, C/4, rest, so the chain left after the
    // call's last copy is C/4's, not C's.
    const bool ramp_ok = C >= 4 * vx_files::DirectIo::kBlock;
    uint64_t chunk_len(uint64_t L, uint64_t a, bool head) const {
        if (!ramp_ok || L < 2 * C) return std::min<uint64_t>(C, L - a);
        const uint64_t q = C / 4, tail_from = (L - C + q - 1) / q * q;
        if (head && a < C) return a < C / 2 ? q : C / 2;
        if (a < tail_from) return std::min<uint64_t>(C, tail_from - a);
        const uint64_t off = a - tail_from;
        return off == 0 ? std::min<uint64_t>(C / 2, L - a) : off == C / 2 ? std::min<uint64_t>(q, L - a) : L - a;
    }
    // chunk lengths of a full-length piece joining now (ramped or not)
    std::vector<uint64_t> schedule(bool ramp) const {
        std::vector<uint64_t> v;
        for (uint64_t a = 0; a < pl;) v.push_back(chunk_len(pl, a, ramp)), a += v.back();
        if (v.empty()) v.push_back(0);
        return v;
    }
    const std::vector<uint64_t> sched_plain = schedule(false), sched_ramp = schedule(true);
    const bool one_round = c->split_one_round && sched_plain.size() == 1;  // every piece is one chunk (pl <= C)
    struct Round {
        int si = -1;
        uint32_t m = 0;
        bool continues = false;
        uint64_t ticket = 0, bytes = 0, max_chunk = 0, t_submit = 0;
    };
    std::deque<Round> formed;  // reads queued, not yet enqueued
    const size_t nslots = c->slots.size();
    const size_t depth = nslots > 1 ? std::min<size_t>(kReadahead, nslots - 1) : 0;
    std::vector<std::vector<vx_files::ReadItem>> items = std::vector<std::vector<vx_files::ReadItem>>(nslots);
    // enqueued rounds: bytes, longest chunk, timing-event index (-1: untimed)
    struct Sent {
        uint64_t bytes, max_chunk;
        long ev;
        bool continues;
    };
    std::vector<Sent> sent;
    size_t measured_upto = 0;  // rounds [0, measured_upto) are in the rates below
    // The copy intake so far: bytes copied over first copy start -> last copy
    // end (a copy that waited for its reads counts the wait).
    double in_bytes = 0, in_ms = 0, in_n = 0;
    float first_cs = -1;
    // every measured copy: (end ms, bytes, longest chunk), for the steady-state
    // intake the next call starts from
    struct CopyEnd {
        double end_ms;
        uint64_t bytes, max_chunk;
    };
    std::vector<CopyEnd> copy_ends;
    std::vector<double> block_ns;         // measured chain per 64-byte block, one per round
    RoundTimeline tlm{c, cp, "vx_verify_files_split"};
    const double pool_threads = sp->cpu_threads;
    // engines claiming from this split at once (vx_split.engines): each takes
    // an equal share of what the pool does not
    const uint64_t engines = std::max<uint32_t>(1, sp->engines);
    std::vector<std::pair<uint64_t, uint64_t>> mine;  // this engine's claims, [lo, hi), in claim order
    std::vector<std::pair<uint64_t, uint64_t>> pool_samples;  // (steady ns, pool_done) at each decision
    static constexpr uint64_t kPoolWindowNs = 4000000;              // the pool's pace: its last 4 ms
    const double thread_rate0 = c->split_pool_thread_rate[regime].any() ? c->split_pool_thread_rate[regime].get(c->split_learn)
                                : sp->cpu_thread_rate > 0    ? sp->cpu_thread_rate
                                                             : 2.2e9;
    const double pool_rate0 = pool_threads * thread_rate0 / (double)pl;
    double last_p = 0;  // the pool's pace at the last decision
    // the first group's predicted ends (call clock, ms; the engine's without
    // the learned lag) and the engine's span, and whether any later group
    // joined: the lag's sample
    double first_end_ms = -1, first_pool_end_ms = -1, first_span_ms = 0, lag_used = 0;
    bool later_group = false;

    // Fold newly finished rounds into the copy and chain rates (events are
    // queried, never waited for).
    size_t copied_upto = 0;  // rounds whose copy is in the intake above
    void measure() {
        // copies as soon as they end (the first rate arrives a kernel earlier)
        while (copied_upto < sent.size()) {
            const Sent& r = sent[copied_upto];
            if (r.ev >= 0) {
                const size_t e = 3 * (size_t)r.ev;
                if (hipEventQuery(c->copy_ev[e + 1]) != hipSuccess) break;
                float cs = 0, ce = 0;
                if (hipEventElapsedTime(&cs, c->copy_ev[0], c->copy_ev[e]) == hipSuccess &&
                    hipEventElapsedTime(&ce, c->copy_ev[0], c->copy_ev[e + 1]) == hipSuccess) {
                    if (first_cs < 0) first_cs = cs;
                    in_bytes += (double)r.bytes;
                    in_ms = (double)ce - (double)first_cs;
                    in_n += 1;
                    copy_ends.push_back(CopyEnd{(double)ce, r.bytes, r.max_chunk});
                }
            }
            ++copied_upto;
        }
        // kernels: the chain per block, and which rounds are done
        while (measured_upto < sent.size()) {
            const Sent& r = sent[measured_upto];
            if (r.ev < 0) {
                ++measured_upto;
                continue;
            }
            const size_t e = 3 * (size_t)r.ev;
            if (hipEventQuery(c->copy_ev[e + 2]) != hipSuccess) break;  // kernel not done yet
            float k0 = 0, k1 = 0, ce = 0;
            // the kernel starts after its copy and, when its lanes continue, after
            // the previous round's kernel
            long prev = -1;
            for (size_t k = measured_upto; r.continues && k-- > 0;)
                if (sent[k].ev >= 0) {
                    prev = sent[k].ev;
                    break;
                }
            if (hipEventElapsedTime(&ce, c->copy_ev[0], c->copy_ev[e + 1]) == hipSuccess &&
                hipEventElapsedTime(&k1, c->copy_ev[0], c->copy_ev[e + 2]) == hipSuccess) {
                if (prev >= 0) (void)hipEventElapsedTime(&k0, c->copy_ev[0], c->copy_ev[3 * (size_t)prev + 2]);
                const double kern_ms = (double)k1 - std::max<double>(ce, prev >= 0 ? k0 : 0.0);
                const double blocks = (double)((r.max_chunk + 63) / 64);
                if (kern_ms > 0 && blocks > 0) block_ns.push_back(kern_ms * 1e6 / blocks);
            }
            ++measured_upto;
        }
    }
    // How many pieces to take now (0..room).
    // mode 0: a round after the first (no group until both sides have rates);
    // 1: the first round (the cold-start answer); 2: nothing is in flight and
    // the rates are not all in: decide with what there is.
    uint64_t decide(uint64_t room, int mode, bool* measured) {
        measure();
        const uint64_t w = __atomic_load_n(&sp->word, __ATOMIC_ACQUIRE);
        const uint64_t head = w & 0xffffffffull, stop = w >> 32;
        const uint64_t unclaimed = stop > head ? stop - head : 0;
        if (unclaimed == 0 || room == 0) return 0;
        const uint64_t done = __atomic_load_n(&sp->pool_done, __ATOMIC_ACQUIRE);
        const uint64_t now = vx_files::Readers::now_ns();
        const double el = ((double)now - (double)sp->start_ns) * 1e-9;
        const bool pool_measured = pool_threads == 0 || (done >= std::max(4.0, pool_threads) && el > 0);
        // The pool's rate over the last few ms (its start-up — threads
        // spawning, first pieces — is not its pace), or since the start.
        double p = pool_threads == 0 ? 0.0 : pool_measured ? (double)done / el : pool_rate0;
        bool windowed = pool_threads == 0;
        for (size_t k = pool_samples.size(); pool_measured && pool_threads > 0 && k-- > 0;) {
            const auto& sm = pool_samples[k];
            if (now - sm.first >= kPoolWindowNs) {
                if (done > sm.second) p = (double)(done - sm.second) / ((double)(now - sm.first) * 1e-9);
                windowed = done > sm.second;
                break;
            }
        }
        pool_samples.emplace_back(now, done);
        // A later group needs the pool's pace over a window (not its start-up)
        // and the engine's intake over two copies.
        *measured = in_n >= 2 && windowed;
        // The first group is decided before the pool has a pace: a rate since
        // the start is mostly its start-up, so it never goes below the rate the
        // caller measured alone (an over-claim cannot be handed back; an
        // under-claim is topped up once the rates are in).  Pieces that fit one
        // round (a group costs one round, not a piece's whole chain) keep
        // deciding so until the rates are in, rather than draining the pipeline.
        const bool cold = mode == 1 || (mode == 0 && one_round && !*measured);
        if (cold && pool_threads > 0) p = std::max(p, pool_rate0);
        // With the engine idle (mode 2), a pool that has finished nothing for
        // two of its piece times (at least the window) while pieces are still
        // unclaimed is held up — vortex's rayon pool also hashes downloads —
        // so it counts as stopped and the engine takes what it can, instead
        // of leaving the rest to it.
        if (mode == 2 && pool_threads > 0 && unclaimed > 0) {
            const uint64_t win = std::max<uint64_t>(kPoolWindowNs, (uint64_t)(2e9 * (double)pl / thread_rate0));
            for (size_t k = pool_samples.size() - 1; k-- > 0;)  // (the last sample is this call's)
                if (now - pool_samples[k].first >= win) {
                    if (pool_samples[k].second == done) p = 0;
                    break;
                }
        }
        // pieces the pool holds count half done
        const double in_hand = 0.5 * ((double)(head - first) - (double)std::min<uint64_t>(done, head - first));
        // The engine's chain per block is a property of the kernel, known within
        // a few % before any round of this call ends (kChainBlock); waiting for
        // a kernel end put the first measured group a whole round later.
        if (!*measured && !cold && mode == 0) return 0;
        if (windowed) last_p = p;
        const double rin = in_n >= 2 && in_ms > 0 ? in_bytes / (in_ms * 1e-3)
                           : c->split_rin[regime].any() ? (c->split_learn ? c->split_rin[regime].top() : c->split_rin[regime].get(0))
                                                  : kPcieRate;
        double bns = c->split_bns[regime].any() ? c->split_bns[regime].get(c->split_learn) : kChainBlock * 1e9;
        if (!block_ns.empty()) {
            std::vector<double> b = block_ns;
            std::nth_element(b.begin(), b.begin() + b.size() / 2, b.end());
            bns = b[b.size() / 2];
        }
        auto round_s = [&](double bytes, uint64_t chunk) {
            return std::max(bytes / rin, (double)((chunk + 63) / 64) * bns * 1e-9);
        };
        // rounds queued ahead of the new group (enqueued and not finished, or
        // formed), in order; nothing sent yet: the first round's read too
        double t_queued = 0;
        uint64_t last_k = 0;  // the longest chunk of the last round queued
        for (size_t k = measured_upto; k < sent.size(); ++k)
            t_queued += round_s((double)sent[k].bytes, sent[k].max_chunk), last_k = sent[k].max_chunk;
        for (const Round& r : formed) t_queued += round_s((double)r.bytes, r.max_chunk), last_k = r.max_chunk;
        // future rounds of the active lanes: bytes per round index
        std::vector<double> fut;
        std::vector<uint64_t> fut_max;  // each future round's longest chunk
        for (const Lane& l : act) {
            const uint64_t L = plen(l.piece);
            uint64_t a = l.a;
            for (size_t r = 0; a < L; ++r) {
                const uint64_t k = chunk_len(L, a, l.ramp);
                if (fut.size() <= r) fut.resize(r + 1, 0.0), fut_max.resize(r + 1, 0);
                fut[r] += (double)k;
                fut_max[r] = std::max(fut_max[r], k);
                a += k;
            }
        }
        const std::vector<uint64_t>& js = mode == 1 ? sched_ramp : sched_plain;
        // (the lag from three calls on: the median of one or two is their noise)
        lag_used = mode == 1 && c->split_lag_on && c->split_lag[regime].n >= 3 ? c->split_lag[regime].get(c->split_learn) : 0.0;
        // Each round costs max(its bytes over the intake, its chain), copies
        // overlapping the previous round's kernel; after the last copy, the
        // last kernel's chain; before the first, the first round's read.
        const bool first_read = sent.empty() && formed.empty();
        auto t_engine = [&](uint64_t j) {
            double t = t_queued;
            uint64_t k_end = last_k;
            const size_t R = std::max<size_t>(fut.size(), j ? js.size() : 0);
            for (size_t r = 0; r < R; ++r) {
                double b = r < fut.size() ? fut[r] : 0.0;
                uint64_t k = r < fut_max.size() ? fut_max[r] : 0;
                if (j && r < js.size()) b += (double)j * (double)js[r], k = std::max(k, js[r]);
                if (b > 0) t += round_s(b, k) + (r == 0 && first_read ? b / rin : 0.0), k_end = k;
            }
            return t + (double)((k_end + 63) / 64) * bns * 1e-9 + lag_used;
        };
        auto t_pool = [&](uint64_t j) {  // the others take an equal share each
            const double left = (double)unclaimed - (double)(engines * j);
            return p > 0 ? (std::max(0.0, left) + in_hand) / p : std::numeric_limits<double>::infinity();
        };
        // A later group rides the rounds the active lanes still have; one that
        // needs more than one round beyond them adds a tail of rounds that are
        // one chain each with PCIe idle, which a rate misread from a short
        // window (a host-wide stall slows both sides for 10+ ms) cannot repay.
        if (mode == 0 && !act.empty() && js.size() > fut.size() + 1) return 0;
        // the largest j in [0, min(unclaimed, room)] with t_engine(j) <= t_pool(j):
        // t_engine grows with j and t_pool shrinks, so bisect
        auto ok = [&](uint64_t j) { return t_engine(j) <= t_pool(j); };
        uint64_t lo = 0, hi = std::min(engines == 1 ? unclaimed : (unclaimed + engines - 1) / engines, room);
        if (ok(hi)) {
            lo = hi;
        } else if (ok(1)) {
            lo = 1;
            while (lo + 1 < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                (ok(mid) ? lo : hi) = mid;
            }
        }

        // and a later group must shorten the predicted end by a tenth (a group
        // of one-round pieces risks one round, and is a small share of the end)
        if (mode == 0 && !one_round && lo > 0 &&
            std::max(t_engine(lo), t_pool(lo)) > 0.9 * std::max(t_engine(0), t_pool(0)))
            lo = 0;
        c->last_split.push_back(vx_ctx::SplitDecision{
            ((double)vx_files::Readers::now_ns() - (double)c->verify_t0_ns) * 1e-6, p, rin, bns,
            t_engine(lo) * 1e3, t_pool(lo) * 1e3, unclaimed, lo, (uint64_t)act.size(), done, (uint32_t)mode,
            *measured ? 1u : 0u, lag_used * 1e3});
        return lo;
    }

    // Form the next round into a slot: the active lanes' next chunks plus a
    // group claimed now.  1 = formed, 0 = nothing left for the engine,
    // -1 = no slot free (block = false) or an error (rc set).
    bool formed_any = false;
    int form(bool block) {
        auto consume = [this] { fv.consume(); };
        int si = -1;
        for (int attempt = 0;; ++attempt) {
            if ((rc = cp.slot(block, &si, consume)) || si < 0) return -1;
            bool measured = false;
            bool inflight = false;
            for (const Slot& q : c->slots) inflight |= q.state == Slot::INFLIGHT;
            const int mode = !formed_any && attempt == 0 ? 1 : (block && !inflight && formed.empty()) ? 2 : 0;
            const uint64_t j = decide(max_lanes - std::min<uint64_t>(max_lanes, act.size()), mode, &measured);
            if (j > 0 || !act.empty()) {
                Slot& s = c->slots[si];
                reset_fill(s);
                if ((rc = ensure_stage(c, s))) return -1;
                auto& it = items[si];
                it.clear();
                // the round's lanes: the active ones, then the group claimed now
                std::vector<Lane> lanes = act;
                const bool continues = !act.empty();
                if (j) {
                    // alone on the split, the stop is where this engine left it
                    uint64_t old = 0;
                    const uint64_t lo = split_take_tail(sp, j, engines == 1 ? *lowest : UINT64_MAX, &old);
                    if (lo == UINT64_MAX) {
                        rc = fail(VX_EINVAL, "vx_verify_files_split: another engine claims from this split");
                        return -1;
                    }
                    if (lo < old && !mine.empty() && mine.back().first == old)
                        mine.back().first = lo;  // right below the last group: one range (one D2H)
                    else if (lo < old)
                        mine.emplace_back(lo, old);
                    for (uint64_t i = lo; i < old; ++i) lanes.push_back(Lane{i, 0, !formed_any});
                    *lowest = std::min(*lowest, lo);
                    const vx_ctx::SplitDecision& d = c->last_split.back();
                    if (mode == 1) {
                        first_span_ms = d.t_engine_ms - lag_used * 1e3;
                        first_end_ms = d.t_ms + first_span_ms;
                        first_pool_end_ms = d.t_ms + d.t_pool_ms;
                    } else if (lo < old) {
                        later_group = true;
                    }
                }
                // lanes sit one round pitch apart: the round's longest chunk,
                // 4 KiB aligned for O_DIRECT (ramp rounds copy no gaps)
                uint64_t max_chunk = 0;
                for (const Lane& l : lanes) max_chunk = std::max(max_chunk, chunk_len(plen(l.piece), l.a, l.ramp));
                const uint64_t rp = std::max<uint64_t>(vx_files::DirectIo::kBlock,
                                                       align_up(max_chunk, vx_files::DirectIo::kBlock));
                uint32_t m = 0;
                std::vector<Lane> keep;
                // one-chunk pieces are whole pieces in increasing order: runs of
                // them inside one file go out as one pread (as in verify_whole)
                vx_files::Runs runs = rd.runs(one_round && c->split_one_round != 2 ? 4ull << 20 : 0);
                for (const Lane& l : lanes) {
                    const uint64_t L = plen(l.piece), clen = chunk_len(L, l.a, l.ramp);
                    if (one_round)
                        runs.add(it, s.stage.get() + (uint64_t)m * rp, l.piece, clen);
                    else
                        it.push_back(vx_files::ReadItem{s.stage.get() + (uint64_t)m * rp, l.piece, l.a, clen});
                    s.h_offsets[m] = (uint64_t)m * rp;
                    s.h_lens[m] = (uint32_t)clen;
                    s.h_pidx[m] = (uint32_t)(l.piece - first);
                    s.h_poff[m] = l.a;
                    s.h_tlen[m] = L;
                    ++m;
                    if (l.a + clen < L) keep.push_back(Lane{l.piece, l.a + clen, l.ramp});
                }
                act.swap(keep);
                if (m == 0) continue;  // the group came back empty (the pool took the rest)
                formed_any = true;
                s.state = Slot::FILLING;  // reserved until the round is enqueued
                Round r;
                r.si = si;
                r.m = m;
                r.continues = continues;
                r.bytes = s.bytes = (uint64_t)(m - 1) * rp + s.h_lens[m - 1];
                r.max_chunk = max_chunk;
                r.t_submit = vx_files::Readers::now_ns();
                r.ticket = rd.submit(it);
                formed.push_back(r);
                return 1;
            }
            // Nothing to form.  While the rates are not all in, wait for a round
            // in flight and decide again (mode 2 once none is left); with
            // them, the engine is done: the pool takes the rest.
            if (!block || measured || mode == 2) return 0;
            if (inflight) {
                if ((rc = reap(c, true))) return -1;
                consume();
            }
        }
    }

    // The driver: up to `depth` rounds' reads queued ahead of the one enqueued.
    int run() {
        *lowest = end;
        // One-chunk pieces' rounds are whole groups: a smaller round starts the
        // first copy sooner and ends the last kernel sooner (64 KiB pieces: 256 ->
        // 64 MiB rounds, 50.5-52.5 -> 55.9-56.0 GiB/s; tools/split_rules_ab.py),
        // but not below 1,024 lanes, whose kernels run one piece's chain each.
        if (one_round && c->split_round_cap)
            max_lanes = std::min(max_lanes, std::max<uint64_t>(1024, c->split_round_cap / pitch));
        tlm.t_last_enqueue = RoundTimeline::clk::now();
        for (;;) {
            while (formed.size() <= depth) {
                const int f = form(formed.empty());
                if (f <= 0) break;
            }
            if (rc || formed.empty()) break;
            Round r = formed.front();
            formed.pop_front();
            rd.wait(r.ticket);
            rc = cp.round(r.si, r.m, r.continues, false, tlm.timed_copy());
            sent.push_back(Sent{r.bytes, r.max_chunk, tlm.kernel_end(r.si, rc), r.continues});
            tlm.push(r.t_submit, rd.done_ns(r.ticket), r.bytes, 0, r.m, r.continues ? 0u : VX_ROUND_NEW_WINDOW);
            if (rc) break;
        }
        rd.wait();  // error path: no read may still target a stage
        release_filling_slots(c);
        // rows of this engine's pieces, relative to first
        std::vector<std::pair<uint64_t, uint64_t>> rows;
        for (const auto& r : mine) {
            rows.emplace_back(r.first - first, r.second - first);
            for (uint64_t i = r.first; i < r.second; ++i) cp.bytes += plen(i);
        }
        rc = cp.finish_rows(fv.matched_out, rc, fv.bad.data(), rows);
        tlm.fold(rc);
        if (!rc) {
            for (const auto& r : rows)
                for (uint64_t i = r.first; i < r.second; ++i)
                    if (fv.bad[i]) fv.matched_out[i] = 0;
            learn();
        }
        fv.done = 0;
        for (const auto& r : rows) fv.done += r.second - r.first;
        return rc;
    }

    // After a call that succeeded: its figures join the context's (Learned).
    void learn() {
        // the next split call's cold start (this host, this load): this
        // call's figures join the last calls' (Learned)
        measure();
        // the steady-state intake: the full-chunk rounds' bytes over the time
        // from the copy before the first of them to the last one's end (the
        // ramps' short rounds and the chain-bound tail would understate it,
        // and the next call would claim too little)
        {
            size_t a = copy_ends.size(), b = 0;
            for (size_t k = 0; k < copy_ends.size(); ++k)
                if (copy_ends[k].max_chunk >= C) a = std::min(a, k), b = k;
            double bytes = 0;
            for (size_t k = a + 1; k <= b && a < copy_ends.size(); ++k) bytes += (double)copy_ends[k].bytes;
            const double ms = a < b ? copy_ends[b].end_ms - copy_ends[a].end_ms : 0.0;
            if (ms > 0 && bytes > 0) c->split_rin[regime].add(bytes / (ms * 1e-3));
        }
        if (!block_ns.empty()) {
            std::nth_element(block_ns.begin(), block_ns.begin() + block_ns.size() / 2, block_ns.end());
            c->split_bns[regime].add(block_ns[block_ns.size() / 2]);
        }
        if (last_p > 0 && pool_threads > 0) c->split_pool_thread_rate[regime].add(last_p * (double)pl / pool_threads);
        // The lag: how much later than predicted the engine's last kernel
        // ended, less how much later than predicted the pool's last verdict
        // came (vx_split.pool_last_ns), both against the first group's
        // decision.
        double end_ms = -1;
        for (const auto& r : c->last_rounds) end_ms = std::max(end_ms, r.kernel_end_ms);
        if (tlm.anchored && !later_group && engines == 1 && first_end_ms > 0 && end_ms > 0 && first_span_ms > 0) {
            double err = end_ms - first_end_ms;
            bool ok = true;
            if (pool_threads > 0) {
                // A pool still verifying its last pieces is waited for (polled,
                // at most 3x their estimated time + 50 ms): estimating its end
                // instead would miss the stalls that come after the engine's,
                // while counting those before it, and bias the lag up.  A pool
                // that has reported nothing is not waited for.
                uint64_t head = 0, stop = 0, done = 0, last_ns = 0;
                auto load = [&] {
                    const uint64_t w = __atomic_load_n(&sp->word, __ATOMIC_ACQUIRE);
                    head = w & 0xffffffffull, stop = w >> 32;
                    done = __atomic_load_n(&sp->pool_done, __ATOMIC_ACQUIRE);
                    last_ns = __atomic_load_n(&sp->pool_last_ns, __ATOMIC_ACQUIRE);
                };
                auto busy = [&] { return stop > head || done < head - first; };
                load();
                if (busy() && done > 0 && last_p > 0) {
                    const double left = 0.5 * (double)(head - first - std::min(done, head - first)) +
                                        (double)(stop > head ? stop - head : 0);
                    const uint64_t until = vx_files::Readers::now_ns() + (uint64_t)((3.0 * left / last_p + 0.05) * 1e9);
                    while (busy() && vx_files::Readers::now_ns() < until) {
                        std::this_thread::sleep_for(std::chrono::microseconds(200));
                        load();
                    }
                }
                ok = !busy() && last_ns && first_pool_end_ms > 0;
                if (ok) err -= ((double)last_ns - (double)c->verify_t0_ns) * 1e-6 - first_pool_end_ms;
            }
            if (ok) {
                const double v = std::clamp(err, -0.25 * first_span_ms, 0.5 * first_span_ms) * 1e-3;
                c->split_lag[regime].add(v);
            }
        }
    }
};

}  // namespace

int vxe::verify_split(FileVerify& fv, vx_files::Readers& rd, vx_split* sp, uint64_t n, uint32_t pl, uint64_t total,
                      uint64_t C, uint64_t* lowest, int regime) {
    return SplitRun{fv, rd, sp, n, pl, total, C, lowest, regime}.run();
}

extern "C" {

int vx_split_init(vx_split* s, uint64_t first, uint64_t end, uint32_t cpu_threads, double cpu_thread_rate) {
    if (!s || first > end || end > 0xffffffffull) return fail(VX_EINVAL, "vx_split_init: bad range");
    if (!(cpu_thread_rate >= 0)) return fail(VX_EINVAL, "vx_split_init: cpu_thread_rate must be >= 0");
    *s = vx_split{};
    s->first = first;
    s->end = end;
    s->cpu_threads = cpu_threads;
    s->cpu_thread_rate = cpu_thread_rate;
    s->start_ns = vx_files::Readers::now_ns();
    __atomic_store_n(&s->word, first | (end << 32), __ATOMIC_RELEASE);
    return 0;
}

int64_t vx_split_claim(vx_split* s) {
    if (!s) return -1;
    uint64_t w = __atomic_load_n(&s->word, __ATOMIC_ACQUIRE);
    for (;;) {
        const uint64_t head = w & 0xffffffffull, stop = w >> 32;
        if (head >= stop) return -1;
        if (__atomic_compare_exchange_n(&s->word, &w, w + 1, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE))
            return (int64_t)head;
    }
}

void vx_split_done(vx_split* s, uint64_t pieces) {
    if (!s) return;
    // the latest verdict's time (a later one never moves it back), published
    // with the count
    const uint64_t t = vx_files::Readers::now_ns();
    uint64_t was = __atomic_load_n(&s->pool_last_ns, __ATOMIC_RELAXED);
    while (was < t &&
           !__atomic_compare_exchange_n(&s->pool_last_ns, &was, t, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
    __atomic_fetch_add(&s->pool_done, pieces, __ATOMIC_RELEASE);
}

uint64_t vx_split_boundary(const vx_split* s) {
    return s ? __atomic_load_n(&s->word, __ATOMIC_ACQUIRE) >> 32 : 0;
}

int64_t vx_verify_files_split(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                              uint32_t piece_length, const uint8_t* expected, size_t n_pieces, vx_split* s,
                              uint8_t* matched_out, uint32_t io_threads) {
    if (!s || s->first > s->end || s->end > n_pieces) return fail(VX_EINVAL, "vx_verify_files_split: bad split");
    return verify_files_impl(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces, s->first,
                             s->end - s->first, matched_out, io_threads, s);
}

// The split over several GPUs of one process: one host thread per context,
// each running vx_verify_files_split on the same claim word, which is
// declared for nctx engines so each sizes its groups as one of nctx equal
// takers beside the pool.  io_threads is the total reader count, divided.
int64_t vx_verify_files_split_multi(vx_ctx* const* ctxs, size_t nctx, const char* const* paths,
                                    const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
                                    const uint8_t* expected, size_t n_pieces, vx_split* s, uint8_t* matched_out,
                                    uint32_t io_threads) {
    if (!ctxs || nctx == 0 || nctx > 1024 || !s) return fail(VX_EINVAL, "vx_verify_files_split_multi: bad argument");
    if (int rc = check_contexts(ctxs, nctx, "vx_verify_files_split_multi")) return rc;
    s->engines = (uint32_t)nctx;
    const uint32_t total_io = io_threads ? io_threads : std::max(1u, std::min(16u, usable_cpus()));
    const uint32_t per_ctx = std::max<uint32_t>(1, total_io / (uint32_t)nctx);
    return fan_out(nctx, [&](size_t k) {
        return vx_verify_files_split(ctxs[k], paths, file_lengths, nfiles, piece_length, expected, n_pieces, s,
                                     matched_out, per_ctx);
    });
}

// Host-only cost model of a bulk verify.  One piece is one
// lane and SHA-1 is Merkle-Damgård, so a piece of L bytes is a chain of
// blocks(L) dependent compressions at kChainBlock seconds each on the split
// kernels (the chunked re-verify pipelines its rounds, so the chain, not the
// round count, is what remains); the bytes cross PCIe at kPcieRate.  The call
// takes the larger of the two, a fixed setup, and a fraction of the smaller
// (they overlap, but not perfectly).  The caller's pool: ceil(n / threads)
// rounds of one piece per thread at cpu_thread_rate bytes/s (rayon runs one
// piece per task, torrent.rs:724-740).  Fitted to the grid measured by
// tools/crossover_grid.py on the asm-consumer build
// (profiles/r02/crossover/grid.json: 22 points, 2-16 MiB x 64-4,096 pieces;
// GPU predictions within 5 %); tests/test_abi.py checks the fit and every
// decision against that file.  use_gpu asks for a 10 % margin: near a tie the
// caller's own pool is the safe choice.
int vx_plan_verify(uint64_t n_pieces, uint32_t piece_length, uint64_t total_length, uint32_t cpu_threads,
                   double cpu_thread_rate, vx_plan* out) {
    return vx_plan_verify_gpus(n_pieces, piece_length, total_length, cpu_threads, cpu_thread_rate, 1, out);
}

// The same model over n_gpus contexts (vx_verify_files_multi):
// each GPU's share of the bytes crosses its own PCIe link, so the transfer
// term divides by n_gpus; one piece's chain does not shrink, which is why a
// host with many cores can keep its pool against any number of GPUs when the
// pieces are long (INTEGRATION.md "A whole node is a different host").
namespace {
constexpr double kSetup = 1.5e-3;
constexpr double kOverlapLoss = 0.08, kMargin = 1.1;
constexpr double kBatchLatency = 1e-3;  // launch, H2D of a small batch, D2H, poll
// A split runs the GPU side's reads beside the pool's hashing on the same
// host.  The pool is sized to leave the engine's readers their cores (the
// caller passes its size; 12 of 16 threads beside 8 readers measured stable);
// beside the engine it hashes at kSplitPool of its per-thread rate alone, and
// the GPU side's bytes move at kSplitLink of the link rate (page-cache reads,
// stage writes and the DMA share host memory with the pool's hashing).  Fitted
// to the warm config-5 split over three boxes (profiles/r05/split/: GPU side
// 36-43 GB/s, the 12-thread pool at 0.85-0.98 of its rate alone), then refit
// on four HEAD bench runs with the copy stream and huge-page stages
// (refit_r05_bench.json: GPU side 38-39.5 GiB/s at its largest share, the pool
// at 0.74-0.85 of its rate alone, median 0.80; at 0.85 the point with 10 % more
// GPU pieces won on all four, by 1-16 %).
constexpr double kSplitLink = 0.74, kSplitPool = 0.80;

// The GPU path over `bytes` bytes of pieces piece_length long, over n_gpus links
// at `link` of the PCIe rate.
void plan_gpu(double L, double bytes, uint32_t n_gpus, vx_plan* out, double link = 1.0) {
    out->gpu_chain_s = std::ceil((L + 9) / 64) * kChainBlock;
    out->gpu_transfer_s = bytes / (kPcieRate * link) / std::max<uint32_t>(1, n_gpus);
    out->gpu_s = std::max(out->gpu_transfer_s, out->gpu_chain_s) + kSetup +
                 kOverlapLoss * std::min(out->gpu_transfer_s, out->gpu_chain_s);
}
}  // namespace

int vx_plan_verify_gpus(uint64_t n_pieces, uint32_t piece_length, uint64_t total_length, uint32_t cpu_threads,
                        double cpu_thread_rate, uint32_t n_gpus, vx_plan* out) {
    if (!out || piece_length == 0) return fail(VX_EINVAL, "vx_plan_verify: bad argument");
    if (n_pieces != (total_length + piece_length - 1) / piece_length)
        return fail(VX_EINVAL, "vx_plan_verify: n_pieces does not match total_length");
    const double threads = cpu_threads ? cpu_threads : 16;
    const double rate = cpu_thread_rate > 0 ? cpu_thread_rate : 2.2e9;
    const double L = piece_length;
    *out = vx_plan{};
    if (n_pieces == 0) return 0;
    plan_gpu(L, (double)total_length, n_gpus, out);
    out->cpu_s = std::ceil((double)n_pieces / threads) * (L / rate);
    out->piece_latency_s = out->gpu_chain_s + kBatchLatency;
    out->cpu_piece_latency_s = L / rate;
    out->use_gpu = out->gpu_s * kMargin < out->cpu_s ? 1 : 0;
    return 0;
}

// The split of one bulk verify between the GPUs (the tail of the piece range)
// and the caller's pool (the head), run at once: the GPU side's time is the
// model above over its bytes at kSplitLink of the link; the pool's is its
// pieces in rounds of one piece per thread.  Every split k = 0..n is scored by
// the slower side and the fastest wins; unless it beats the pool alone by
// kMargin the pool keeps everything.
int vx_plan_verify_split(uint64_t n_pieces, uint32_t piece_length, uint64_t total_length, uint32_t cpu_threads,
                         double cpu_thread_rate, uint32_t n_gpus, uint64_t* gpu_first, uint64_t* gpu_count,
                         vx_plan* out) {
    if (!gpu_first || !gpu_count || piece_length == 0) return fail(VX_EINVAL, "vx_plan_verify_split: bad argument");
    if (n_pieces != (total_length + piece_length - 1) / piece_length)
        return fail(VX_EINVAL, "vx_plan_verify_split: n_pieces does not match total_length");
    const double threads = cpu_threads ? cpu_threads : 16;
    const double rate = cpu_thread_rate > 0 ? cpu_thread_rate : 2.2e9;
    const double L = piece_length;
    const double last = n_pieces ? (double)(total_length - (n_pieces - 1) * (uint64_t)piece_length) : 0.0;
    auto gpu_bytes = [&](uint64_t k) { return k ? (double)(k - 1) * L + last : 0.0; };
    auto cpu_time = [&](uint64_t k) {  // the pool's n - k pieces, one per thread per round
        if (k >= n_pieces) return 0.0;
        return std::ceil((double)(n_pieces - k) / threads) * (L / (k ? rate * kSplitPool : rate));
    };
    vx_plan g{};
    auto gpu_time = [&](uint64_t k) {
        plan_gpu(L, gpu_bytes(k), n_gpus, &g, k < n_pieces ? kSplitLink : 1.0);
        return g.gpu_s;
    };
    uint64_t best_k = 0;
    double best_t = cpu_time(0);
    const double pool_alone = best_t;
    auto consider = [&](uint64_t k) {
        if (k < 1 || k > n_pieces) return;
        const double t = std::max(gpu_time(k), cpu_time(k));
        if (t < best_t || (t == best_t && k < best_k)) best_t = t, best_k = k;
    };
    // On 1 <= k < n the GPU side's time never falls as k grows and the
    // pool's never rises, so the slower side is least where they cross:
    // bisect for the first k whose GPU time reaches the pool's, then score it,
    // its neighbours and k = n (whose link has no pool beside it).  A scan of
    // every k cost a multi-TB torrent of 16 KiB pieces ~10^7 evaluations.
    if (n_pieces > 1) {
        uint64_t lo = 1, hi = n_pieces - 1;
        if (gpu_time(hi) < cpu_time(hi)) {
            lo = hi;
        } else {
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (gpu_time(mid) >= cpu_time(mid)) hi = mid;
                else lo = mid + 1;
            }
        }
        for (uint64_t k = lo > 2 ? lo - 2 : 1; k <= std::min<uint64_t>(n_pieces - 1, lo + 2); ++k) consider(k);
        // left of the crossing the pool's side binds, and its time is a step
        // function (rounds of `threads` pieces): the step's first k ties it
        if (lo > 1) {
            const uint64_t m = (uint64_t)std::ceil((double)(n_pieces - (lo - 1)) / threads);
            const uint64_t k0 = n_pieces > m * (uint64_t)threads ? n_pieces - m * (uint64_t)threads : 1;
            consider(std::max<uint64_t>(1, k0));
        }
    }
    consider(n_pieces);
    if (best_k && best_t * kMargin >= pool_alone) best_k = 0;
    *gpu_count = best_k;
    *gpu_first = n_pieces - best_k;
    if (out) {
        *out = vx_plan{};
        if (best_k) plan_gpu(L, gpu_bytes(best_k), n_gpus, out, best_k < n_pieces ? kSplitLink : 1.0);
        out->cpu_s = cpu_time(best_k);
        vx_plan one{};
        plan_gpu(L, L, 1, &one);  // the download path's figures do not depend on the split
        out->piece_latency_s = one.gpu_chain_s + kBatchLatency;
        out->cpu_piece_latency_s = L / rate;
        out->use_gpu = best_k ? 1 : 0;
    }
    return 0;
}

#ifdef VX_TEST_HOOKS
void vx_tuning_split_rules(vx_ctx* c, int one_round, uint64_t round_cap, int lag, int learn) {
    if (!c) return;
    c->split_lag_on = lag ? 1 : 0;
    c->split_learn = learn ? 1 : 0;
    c->split_one_round = one_round == 2 ? 2 : one_round ? 1 : 0;
    c->split_round_cap = round_cap;
}
#endif

uint64_t vx_tuning_split_take_tail(vx_split* s, uint64_t k, uint64_t* was) {
    return s ? split_take_tail(s, k, UINT64_MAX, was) : 0;
}

size_t vx_tuning_last_split(const vx_ctx* c, double* out, size_t max) {
    if (!c) return 0;
    const size_t k = std::min(max, c->last_split.size());
    for (size_t i = 0; i < k && out; ++i) {
        const auto& d = c->last_split[i];
        const double row[13] = {d.t_ms, d.pool_rate, d.engine_rate, d.block_ns, d.t_engine_ms, d.t_pool_ms,
                                (double)d.unclaimed, (double)d.group, (double)d.lanes, (double)d.pool_done,
                                (double)d.mode, (double)d.measured, d.lag_ms};
        std::memcpy(out + 13 * i, row, sizeof row);
    }
    return c->last_split.size();
}

}  // extern "C"
