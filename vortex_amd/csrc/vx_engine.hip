// vx_engine.hip — the context behind the C ABI in include/vx_hash.h.
//
// The library replaces, on the host, what vortex does around its hashing pool:
//  * vx_submit / vx_flush / vx_poll and their v2 and hybrid forms: the
//    scope.spawn → mpsc → try_recv cycle (peer_connection.rs:1145-1158 →
//    torrent.rs:415-442), batched for the GPU: the slot path, vx_slots.hip.
//  * vx_sha1_batch / vx_verify_batch: the par_iter bulk verify
//    (torrent.rs:724-740): here.
//  * vx_sha1_device_*: enqueue the kernels on device-resident batches: here.
//
// Design (DESIGN.md "Host engine"): a context owns `slots` batch slots, each
// with its own HIP stream, a device arena, a pinned staging arena and pinned
// metadata.  Pieces are appended to the filling slot at 256-byte aligned
// offsets: pieces inside a registered (pinned) host range are pulled at launch
// by one gather kernel through the range's device mapping (vx_gather.hip);
// others go through the slot's pinned stage and move with one H2D per
// contiguous run at launch.  On the async path (vx_submit) the stage copy is
// a memcpy at submit; inside a host batch (vx_*_batch) the copies are
// deferred to launch and split over up to 16 short-lived threads, and the call
// waits for every slot before it returns.  Slots on different streams overlap
// copy and compute.  The async path has no internal threads: like the
// reference's loop, it is driven from the caller's thread.
//
// This unit: the error text, context lifecycle, slot and stage allocation and
// warm-up, registration, host batches, stats, vx_sha1_device_*, the tuning and
// synth entries.  The download path is vx_slots.hip, the file re-verify
// vx_reverify.hip, the split and the planner vx_split.hip, BitTorrent v2
// vx_merkle.hip, hybrid torrents vx_hybrid.hip (DESIGN.md "Host engine").
#include "vx_chunk_pipe.hpp"

#ifdef VX_TEST_HOOKS
#include <atomic>
#endif

// The handles' backend over HIP (vx_resources.hpp): the only place the engine
// allocates or frees device or pinned memory, creates or destroys a stream or
// an event, or registers a stage.  The test build counts what is alive
// (vx_tuning_live_resources) and can fail a creation before the runtime is
// asked (vx_tuning_fail_alloc_after): process-wide, so file-scope atomics (the
// _multi calls run one thread per context), not context members.
namespace vx_res::backend {

enum Counted { kDevice, kPinned, kStreams, kEvents };
#ifdef VX_TEST_HOOKS
static std::atomic<int64_t> g_live[4];
static std::atomic<int64_t> g_fail_alloc_after{-1};
// true: this creation is the injected failure (which disarms the hook)
static bool injected_failure() {
    int64_t left = g_fail_alloc_after.load();
    while (left >= 0)
        if (g_fail_alloc_after.compare_exchange_weak(left, left - 1)) return left == 0;
    return false;
}
static void count(Counted what, int by) { g_live[what] += by; }
#else
static bool injected_failure() { return false; }
static void count(Counted, int) {}
#endif
void* device_alloc(uint64_t bytes) {
    void* p = nullptr;
    if (injected_failure() || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    count(kDevice, +1);
    return p;
}
void device_free(void* p) {
    (void)hipFree(p);
    count(kDevice, -1);
}
void* pinned_alloc(uint64_t bytes) {
    void* p = nullptr;
    if (injected_failure() || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    count(kPinned, +1);
    return p;
}
void pinned_free(void* p) {
    (void)hipHostFree(p);
    count(kPinned, -1);
}
hipEvent_t event_create(unsigned flags) {
    hipEvent_t e = nullptr;
    if (injected_failure() || hipEventCreateWithFlags(&e, flags) != hipSuccess) return nullptr;
    count(kEvents, +1);
    return e;
}
void event_destroy(hipEvent_t e) {
    (void)hipEventDestroy(e);
    count(kEvents, -1);
}
hipStream_t stream_create(unsigned flags, const int* priority) {
    hipStream_t s = nullptr;
    if (injected_failure() || (priority ? hipStreamCreateWithPriority(&s, flags, *priority)
                                        : hipStreamCreateWithFlags(&s, flags)) != hipSuccess)
        return nullptr;
    count(kStreams, +1);
    return s;
}
void stream_synchronize(hipStream_t s) { (void)hipStreamSynchronize(s); }
void stream_destroy(hipStream_t s) {
    (void)hipStreamDestroy(s);
    count(kStreams, -1);
}
bool stage_register(void* p, uint64_t bytes) {
    if (injected_failure() || hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) return false;
    count(kPinned, +1);
    return true;
}
void stage_unregister(void* p) {
    (void)hipHostUnregister(p);
    count(kPinned, -1);
}

}  // namespace vx_res::backend

namespace vxe {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return VX_EDEVICE;
}

// Pieces (lanes) a slot's metadata holds: the async batch size, or enough
// chunk lanes to fill the arena with kMinChunk-byte chunks (the chunked paths
// of §6.3/§6.4 put one chunk per lane), whichever is larger.
constexpr uint64_t kMinChunk = 64 * 1024;
uint32_t slot_capacity(const vx_config* cfg) {
    return (uint32_t)std::min<uint64_t>(1u << 20, std::max<uint64_t>(cfg->batch_pieces, cfg->slot_bytes / kMinChunk));
}

int set_device(const vx_ctx* c) {
    VX_HIP(hipSetDevice(c->cfg.device));
    return 0;
}

// True if [p, p+len) lies in one registered range; *dev (optional) gets the
// device-mapped address of p.
bool is_registered(const vx_ctx* c, const void* p, size_t len, const uint8_t** dev) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto hit = c->registered_at.find(a);
    if (hit != c->registered_at.end() && len <= hit->second.len) {
        if (dev) *dev = hit->second.dev;
        return true;
    }
    auto it = c->registered.upper_bound(a);
    if (it == c->registered.begin()) return false;
    --it;
    if (!(a >= it->first && a + len <= it->first + it->second.len)) return false;
    if (dev) *dev = it->second.dev + (a - it->first);
    return true;
}

int alloc_slot(Slot& s, uint64_t arena, uint32_t cap) {
    s.arena_cap = arena;
    s.cap = cap;
    if (!s.stream.make(hipStreamNonBlocking) || !s.done.make(hipEventDisableTiming) ||
        !s.copied.make(hipEventDisableTiming))
        return fail(VX_EDEVICE, "vx_create: stream or event creation failed");
    if (!s.d_arena.reserve(arena)) return fail(VX_ENOMEM, "device arena allocation failed");
    // The pinned stage is allocated on first use (ensure_stage): a caller that
    // registers its buffer pool never stages, and pinning slot_bytes of host
    // memory per slot up front would cost as much as the HBM arena.
    // offsets | chunk offsets | total lens | gather sources | lens | piece rows |
    // gather tile prefix (cap+1) | expected | digests | verdicts
    const size_t meta = (size_t)cap * (8 + 8 + 8 + 8 + 4 + 4 + 4 + 20 + 20 + 1) + 64;
    if (!s.h_meta.reserve(meta)) return fail(VX_ENOMEM, "pinned metadata allocation failed");
    if (!s.d_meta.reserve(meta)) return fail(VX_ENOMEM, "device metadata allocation failed");
    auto carve = [cap](uint8_t* b, uint64_t*& off, uint64_t*& poff, uint64_t*& tlen, uint64_t*& src,
                       uint32_t*& lens, uint32_t*& pidx, uint32_t*& tfirst, uint8_t*& exp, uint8_t*& dig,
                       uint8_t*& m) {
        size_t at = 0;
        auto take = [&](size_t bytes) {
            uint8_t* p = b + at;
            at += bytes;
            return p;
        };
        off = reinterpret_cast<uint64_t*>(take((size_t)cap * 8));
        poff = reinterpret_cast<uint64_t*>(take((size_t)cap * 8));
        tlen = reinterpret_cast<uint64_t*>(take((size_t)cap * 8));
        src = reinterpret_cast<uint64_t*>(take((size_t)cap * 8));
        lens = reinterpret_cast<uint32_t*>(take((size_t)cap * 4));
        pidx = reinterpret_cast<uint32_t*>(take((size_t)cap * 4));
        tfirst = reinterpret_cast<uint32_t*>(take((size_t)cap * 4 + 4));
        exp = take((size_t)cap * 20);
        dig = take((size_t)cap * 20);
        m = take(cap);
    };
    carve(s.h_meta.get(), s.h_offsets, s.h_poff, s.h_tlen, s.h_src, s.h_lens, s.h_pidx, s.h_tfirst, s.h_expected,
          s.h_digests, s.h_matched);
    carve(s.d_meta.get(), s.d_offsets, s.d_poff, s.d_tlen, s.d_src, s.d_lens, s.d_pidx, s.d_tfirst, s.d_expected,
          s.d_digests, s.d_matched);
    s.h_tfirst[0] = 0;
    s.tags.reserve(cap);
    return 0;
}

// Pinned stage of slot s (unregistered pieces, file reads), allocated on first use.
int ensure_stage(const vx_ctx* c, Slot& s) {
    if (s.stage) return 0;
    if (!s.stage.make(s.arena_cap, c->stage_huge != 0)) return fail(VX_ENOMEM, "pinned stage allocation failed");
    return 0;
}

void reset_fill(Slot& s) {
    s.tags.clear();
    s.runs.clear();
    s.druns.clear();
    s.staged.clear();
    s.staged_bytes = 0;
    s.n = 0;
    s.bytes = 0;
    s.gtiles = 0;
    if (s.h_tfirst) s.h_tfirst[0] = 0;
    s.uniform = true;
    s.has_expected = false;
    s.use_table = false;
    s.kind = Slot::Kind::V1;
    s.v2.kmax = 0;
    s.hy.total = 0;
    s.hy.rows.clear();
    s.all_mapped = true;
}

// CPUs this process may run on (the container's or cgroup's share, not the
// machine's: hardware_concurrency reports every CPU of a large host).
unsigned usable_cpus() {
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) {
        const int n = CPU_COUNT(&set);
        if (n > 0) return (unsigned)n;
    }
    return std::max(1u, std::thread::hardware_concurrency());
}

// Run every command type a batch uses once on every slot stream, in the
// launch pattern of vx_slots.hip's launch_v1 (cross-slot copy chain, large and small
// H2D, both default kernels, D2H).  The HIP runtime sets up the hardware
// queues and copy paths behind a stream on first use, and that blocked the
// host for ~8 ms inside hipMemcpyAsync on the first two slots of the first
// batches (profiles/r01/e2e_first_use/); paying it here keeps it off the
// batch path.
int warm_slots(vx_ctx* c) {
    int prev = -1;
    for (int si = 0; si < (int)c->slots.size(); ++si) {
        Slot& s = c->slots[si];
        hipStream_t st = s.stream;
        if (prev >= 0) VX_HIP(hipStreamWaitEvent(st, c->slots[prev].copied, 0));
        VX_HIP(hipMemcpyAsync(s.d_arena.get(), s.h_meta.get(), std::min<uint64_t>(s.arena_cap, (uint64_t)s.cap * 85),
                              hipMemcpyHostToDevice, st));
        VX_HIP(hipMemcpyAsync(s.d_expected, s.h_expected, 20, hipMemcpyHostToDevice, st));
        VX_HIP(hipEventRecord(s.copied, st));
        hipError_t e = vx::launch_uniform(s.d_arena.get(), kAlign, 64, 1, s.d_digests, s.d_expected, s.d_matched, st,
                                          vx::kUniformDefault, nullptr);
        if (e == hipSuccess) {
            s.h_offsets[0] = 0;
            s.h_lens[0] = 64;
            VX_HIP(hipMemcpyAsync(s.d_offsets, s.h_offsets, 8, hipMemcpyHostToDevice, st));
            VX_HIP(hipMemcpyAsync(s.d_lens, s.h_lens, 4, hipMemcpyHostToDevice, st));
            e = vx::launch_ragged(s.d_arena.get(), s.d_offsets, s.d_lens, nullptr, 1, s.d_digests, s.d_expected,
                                  s.d_matched, st, vx::kUniformDefault, nullptr);
        }
        if (e != hipSuccess) return hip_fail(e, "vx_create: warm-up launch");
        VX_HIP(hipMemcpyAsync(s.h_digests, s.d_digests, 20, hipMemcpyDeviceToHost, st));
        VX_HIP(hipMemcpyAsync(s.h_matched, s.d_matched, 1, hipMemcpyDeviceToHost, st));
        VX_HIP(hipEventRecord(s.done, st));
        prev = si;
    }
    for (auto& s : c->slots) VX_HIP(hipStreamSynchronize(s.stream));
    c->last_launched = prev;
    return 0;
}

// Strided host batches of long pieces: every piece inside
// one registered range at a constant host stride, all of one length except
// possibly a shorter last piece — a bulk verify over a contiguous host copy
// of the torrent (torrent.rs:724-740), or the bench's e2e sample.  Round k of
// a window moves bytes [k*C, (k+1)*C) of each of its pieces with ONE
// hipMemcpy2DAsync (source pitch = host stride; 53 GiB/s like a flat copy,
// profiles/r01/h2d/h2d2d.json), and the chunk kernel continues each piece's
// state.  So the transfer is back to back and only the last round's short
// chain trails it, instead of a whole-piece chain per slot.
bool strided_batch(const vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, size_t n,
                   uint64_t* host_stride) {
    const uint64_t C = c->cfg.batch_chunk;
    if (n == 0 || C == 0 || c->slots[0].arena_cap < C) return false;
    const uint32_t L = lens[0];
    if (L < 2 * C || L > c->cfg.max_piece_len || lens[n - 1] == 0 || lens[n - 1] > L) return false;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(ptrs[0]);
    const uintptr_t hs = n > 1 ? reinterpret_cast<uintptr_t>(ptrs[1]) - p0 : L;
    if (hs < L || hs > (1ull << 40)) return false;
    for (size_t i = 0; i + 1 < n; ++i)
        if (lens[i] != L || reinterpret_cast<uintptr_t>(ptrs[i]) != p0 + i * hs) return false;
    if (reinterpret_cast<uintptr_t>(ptrs[n - 1]) != p0 + (n - 1) * hs) return false;
    if (!is_registered(c, ptrs[0], (n - 1) * hs + lens[n - 1])) return false;
    *host_stride = hs;
    return true;
}

int batch_chunked(vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, const uint8_t* expected, size_t n,
                  uint8_t* matched_out, uint8_t* digests_out, uint64_t hs) {
    const uint64_t C = c->cfg.batch_chunk;
    const uint64_t L = lens[0], Llast = lens[n - 1];
    const uint8_t* base = ptrs[0];
    ChunkPipe cp(c);
    int rc = cp.open(n, expected, "batch");
    for (size_t i = 0; i < n; ++i) cp.bytes += lens[i];
    const Slot& s0 = c->slots[0];
    const uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>(s0.cap, s0.arena_cap / C));
    const uint64_t rounds = (L + C - 1) / C;
    for (uint64_t w0 = 0; w0 < n && !rc; w0 += W) {
        const uint64_t w1 = std::min<uint64_t>(n, w0 + W);
        const bool short_last = w1 == n && Llast != L;
        const uint64_t full_rows = (w1 - w0) - (short_last ? 1 : 0);
        for (uint64_t k = 0; k < rounds && !rc; ++k) {
            const uint64_t a = k * C;
            const uint64_t width = std::min<uint64_t>(C, L - a);   // every full-length row
            const uint64_t dpitch = align_up(width, kAlign);       // <= C
            const uint64_t last_w = short_last && a < Llast ? std::min<uint64_t>(C, Llast - a) : 0;
            const uint32_t m = (uint32_t)(full_rows + (last_w ? 1 : 0));
            if (m == 0) continue;
            const int si = cp.free_slot([] {});
            if (si < 0) {
                rc = si;
                break;
            }
            Slot& s = c->slots[si];
            reset_fill(s);
            for (uint32_t r = 0; r < m; ++r) {
                const bool is_last = r == full_rows;
                s.h_offsets[r] = (uint64_t)r * dpitch;
                s.h_lens[r] = (uint32_t)(is_last ? last_w : width);
                s.h_pidx[r] = (uint32_t)(is_last ? n - 1 : w0 + r);
                s.h_poff[r] = a;
                s.h_tlen[r] = is_last ? Llast : L;
            }
            rc = cp.round(si, m, k > 0, false, [&](Slot& sl, hipStream_t st) {
                if (full_rows && hipMemcpy2DAsync(sl.d_arena.get(), dpitch, base + w0 * hs + a, hs, width, full_rows,
                                                  hipMemcpyHostToDevice, st) != hipSuccess)
                    return fail(VX_EDEVICE, "batch: chunk 2D H2D failed");
                if (last_w && hipMemcpyAsync(sl.d_arena.get() + full_rows * dpitch, ptrs[n - 1] + a, last_w,
                                             hipMemcpyHostToDevice, st) != hipSuccess)
                    return fail(VX_EDEVICE, "batch: chunk H2D failed");
                return 0;
            });
        }
        cp.end_window();
    }
    return cp.finish(matched_out, digests_out, rc);
}

// Registered host batches that are not strided: pieces in
// any registered buffers (vortex's pool has one mmap per buffer,
// buf_pool.rs:92-98), 16-byte aligned, any lengths, the longest >= 2 chunks.
// Same rounds as batch_chunked, but each round's bytes are pulled by the
// gather kernel (vx_gather.hip) through the buffers' device mappings: lane m
// reads bytes [a, a + C) of its piece.
bool gather_batch(const vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, size_t n,
                  std::vector<const uint8_t*>& dev) {
    const uint64_t C = c->cfg.batch_chunk;
    if (n == 0 || C == 0 || c->slots[0].arena_cap < C) return false;
    uint32_t max_len = 0;
    dev.assign(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        if (lens[i] > c->cfg.max_piece_len) return false;
        max_len = std::max(max_len, lens[i]);
        if (lens[i] == 0) continue;
        if ((reinterpret_cast<uintptr_t>(ptrs[i]) & 15) || !is_registered(c, ptrs[i], lens[i], &dev[i]))
            return false;
    }
    return max_len >= 2 * C;
}

int batch_chunked_gather(vx_ctx* c, const uint32_t* lens, const uint8_t* expected, size_t n, uint8_t* matched_out,
                         uint8_t* digests_out, const std::vector<const uint8_t*>& dev) {
    const uint64_t C = c->cfg.batch_chunk;
    ChunkPipe cp(c);
    int rc = cp.open(n, expected, "batch");
    for (size_t i = 0; i < n; ++i) cp.bytes += lens[i];
    const Slot& s0 = c->slots[0];
    const uint64_t W = std::max<uint64_t>(1, std::min<uint64_t>(s0.cap, s0.arena_cap / C));
    // Pieces go longest first (stable, so equal lengths keep the caller's
    // order).  Every round is one C-byte chain whatever its lane count; in
    // caller-order windows every window with a long piece paid that whole
    // chain while its late rounds carried a few MiB each (config 3 from host,
    // DESIGN.md §6.4; that variant was removed in round 4, EXPERIMENTS.md).
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return lens[x] > lens[y]; });
    auto gather_copy = [&](uint32_t m, uint32_t tiles) {
        return [&, m, tiles](Slot& sl, hipStream_t st) -> int {
            if (hipMemcpyAsync(sl.d_src, sl.h_src, (size_t)m * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipMemcpyAsync(sl.d_tfirst, sl.h_tfirst, (size_t)(m + 1) * 4, hipMemcpyHostToDevice, st) !=
                    hipSuccess)
                return fail(VX_EDEVICE, "batch: gather table H2D failed");
            hipError_t e = vx::launch_gather(sl.d_src, sl.d_offsets, sl.d_lens, sl.d_tfirst, m, tiles, sl.d_arena.get(), st);
            if (e != hipSuccess) return hip_fail(e, "batch: gather launch");
            c->stats.gather_tiles += tiles;
            return 0;
        };
    };
    // Streaming rounds: a piece takes a lane from its first chunk to its
    // last, and new pieces (longest first) join any round until it holds
    // `target` bytes.  So the short pieces ride along the long pieces'
    // later rounds instead of queueing behind them, and no round is a
    // C-byte chain that moves only a few MiB.
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += lens[i];
    const uint64_t max_rounds = std::max<uint64_t>(1, (n ? (uint64_t)lens[order[0]] + C - 1 : 0) / C);
    // Spread evenly over the longest piece's rounds: a round is bound by
    // max(its bytes over PCIe, one C-byte chain), and the batch cannot take
    // fewer rounds than its longest piece has chunks.  (A uniform batch gets
    // target = n*C: every piece in the first round, as a window would.)
    const uint64_t target = std::max<uint64_t>(1, (total + max_rounds - 1) / max_rounds);
    std::vector<std::pair<uint32_t, uint64_t>> act, keep;  // (piece, next offset)
    size_t next = 0;
    while (!rc && (!act.empty() || next < n)) {
        const int si = cp.free_slot([] {});
        if (si < 0) {
            rc = si;
            break;
        }
        Slot& s = c->slots[si];
        reset_fill(s);
        uint32_t m = 0, tiles = 0;
        uint64_t bytes = 0;
        keep.clear();
        auto lane = [&](uint32_t i, uint64_t a) {
            const uint64_t L = lens[i];
            const uint32_t clen = (uint32_t)std::min<uint64_t>(C, L - a);
            s.h_offsets[m] = (uint64_t)m * C;
            s.h_lens[m] = clen;
            s.h_pidx[m] = i;
            s.h_poff[m] = a;
            s.h_tlen[m] = L;
            s.h_src[m] = clen ? reinterpret_cast<uint64_t>(dev[i] + a) : 0;
            tiles += clen ? vx::gather_tiles(clen) : 0;
            s.h_tfirst[m + 1] = tiles;
            ++m;
            bytes += clen;
            if (a + clen < L) keep.emplace_back(i, a + clen);
        };
        const bool continues = !act.empty();
        for (const auto& pa : act) lane(pa.first, pa.second);
        while (next < n && m < W && (bytes < target || m == 0)) lane(order[next++], 0);
        act.swap(keep);
        rc = cp.round(si, m, continues, true, gather_copy(m, tiles));
    }
    return cp.finish(matched_out, digests_out, rc);
}
void release_filling_slots(vx_ctx* c) {
    for (auto& s : c->slots)
        if (s.state == Slot::FILLING) {
            reset_fill(s);
            s.state = Slot::FREE;
        }
}

void wait_and_free_inflight(vx_ctx* c) {
    for (auto& s : c->slots)
        if (s.state == Slot::INFLIGHT) (void)hipEventSynchronize(s.done);
    for (auto& s : c->slots)
        if (s.state == Slot::INFLIGHT) {
            reset_fill(s);
            s.state = Slot::FREE;
        }
}

int begin_bulk_call(vx_ctx* c, const std::string& who, bool need_idle) {
    if (c->pending) return fail(VX_EBUSY, who + ": async pieces pending; drain and poll first");
    if (c->sticky) return c->sticky;
    if (c->filling >= 0) {  // an empty filling slot (pending == 0): hand it back
        c->slots[c->filling].state = Slot::FREE;
        c->filling = -1;
    }
    for (auto& s : c->slots)
        if (need_idle && s.state != Slot::FREE) return fail(VX_EBUSY, who + ": a batch is in flight");
    return 0;
}

// A host batch failed part way (an argument or allocation error at some
// submit, a failed launch, a device error).  The call borrows the caller's
// buffers only until it returns, so every slot still reading them — a DMA or
// the gather kernel in flight — is waited for, and every piece of the call
// is dropped: the filling slot is discarded without its deferred stage
// copies, completions already queued are cleared, and pending returns to 0
// (batch_impl starts with nothing pending), so later batches, vx_poll and
// vx_unregister_host_buffer see a clean context.  Only c->done: a bulk call
// submits v1 pieces alone, so the v2 and hybrid queues hold nothing of it.
static void abandon_batch(vx_ctx* c) {
    wait_and_free_inflight(c);
    release_filling_slots(c);
    c->done.clear();
    c->filling = -1;
    c->flush_pending = false;
    c->pending = 0;
}

}  // namespace vxe

using namespace vxe;

extern "C" {

int vx_abi_version(void) { return VX_ABI_VERSION; }

const char* vx_last_error(void) { return g_err.c_str(); }

const char* vx_strerror(int code) {
    switch (code) {
        case VX_OK: return "ok";
        case VX_EINVAL: return "invalid argument";
        case VX_ENOMEM: return "out of memory";
        case VX_ERANGE: return "piece longer than max_piece_len";
        case VX_ENODEV: return "no such device";
        case VX_EDEVICE: return "HIP runtime error";
        case VX_EBUSY: return "busy: work in flight";
        default: return "unknown error";
    }
}

int vx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void vx_config_default(vx_config* cfg, uint32_t max_piece_len) {
    if (!cfg) return;
    cfg->device = 0;
    cfg->max_piece_len = max_piece_len;
    cfg->slots = 4;
    // Throughput of the async path is bytes in flight / batch latency, and a
    // batch's latency is its longest piece's chain (~28 ms at 2 MiB: one lane
    // hashes ~74 MB/s), so slots grow with the piece length: 512 pieces each,
    // 128 MiB to 2 GiB of HBM.  128 pieces per slot held only ~512 lanes in
    // flight over 4 slots; 512 took async 2 MiB pieces 25.7 -> 32.8 GiB/s and
    // 4 MiB 22.3 -> 27.1 (profiles/r01/async/slot_sweep.jsonl).  (The pinned
    // stage is only allocated for unregistered pieces; keeping it at 128 MiB
    // for short pieces keeps their staging memcpy cache-friendly: 256 MiB
    // slots halved the unregistered 16 KiB rate, async_probe.)
    const uint64_t piece = align_up(std::max<uint32_t>(max_piece_len, 1), kAlign);
    cfg->slot_bytes = std::max(piece, std::min<uint64_t>(2ull << 30, std::max<uint64_t>(128ull << 20, piece * 512)));
    cfg->batch_pieces = (uint32_t)std::min<uint64_t>(65536, cfg->slot_bytes / align_up(std::max<uint32_t>(max_piece_len, 1), kAlign));
    cfg->zero_copy = 1;
    cfg->direct_io = 1;
    cfg->batch_chunk = 64 * 1024;
    cfg->verify_chunk = 0;         // per call: verify_chunk_for
    cfg->verify_cold_chunk = 0;
    cfg->verify_ramp = 1;
    cfg->refuse_when_full = 0;
}

int vx_create(const vx_config* cfg, vx_ctx** out) {
    if (!cfg || !out) return fail(VX_EINVAL, "vx_create: NULL argument");
    *out = nullptr;
    if (cfg->max_piece_len == 0 || cfg->slots == 0 || cfg->batch_pieces == 0)
        return fail(VX_EINVAL, "vx_create: max_piece_len, slots and batch_pieces must be > 0");
    if (cfg->slot_bytes < cfg->max_piece_len) return fail(VX_EINVAL, "vx_create: slot_bytes < max_piece_len");
    if (cfg->zero_copy > 1 || cfg->direct_io > 1 || cfg->refuse_when_full > 1)
        return fail(VX_EINVAL, "vx_create: zero_copy, direct_io and refuse_when_full are 0 or 1");
    if (cfg->verify_ramp > 5) return fail(VX_EINVAL, "vx_create: verify_ramp must be 0..5");
    if ((cfg->batch_chunk && (cfg->batch_chunk < 4096 || cfg->batch_chunk % 4096)) ||
        (cfg->verify_chunk && (cfg->verify_chunk < 4096 || cfg->verify_chunk % 4096)) ||
        (cfg->verify_cold_chunk && (cfg->verify_cold_chunk < 4096 || cfg->verify_cold_chunk % 4096)))
        return fail(VX_EINVAL, "vx_create: chunk sizes must be 0 or multiples of 4096");
    // At most 1 GiB: a wrapped negative value from a binding is a huge
    // multiple of 4096.  (A chunk larger than a slot's arena is
    // legal: those calls take the whole-piece path.)
    constexpr uint32_t kMaxChunk = 1u << 30;
    if (cfg->batch_chunk > kMaxChunk || cfg->verify_chunk > kMaxChunk || cfg->verify_cold_chunk > kMaxChunk)
        return fail(VX_EINVAL, "vx_create: chunk sizes must be at most 1 GiB");
    const int ndev = vx_device_count();
    if (cfg->device < 0 || cfg->device >= ndev) return fail(VX_ENODEV, "vx_create: no such HIP device");
    vx_ctx* c = new (std::nothrow) vx_ctx();
    if (!c) return fail(VX_ENOMEM, "vx_create: out of host memory");
    c->cfg = *cfg;
    int rc = set_device(c);
    if (!rc) {
        c->slots.resize(cfg->slots);
        for (auto& s : c->slots) {
            rc = alloc_slot(s, cfg->slot_bytes, slot_capacity(cfg));
            if (rc) break;
        }
    }
    if (!rc) rc = warm_slots(c);
    if (rc) {
        delete c;  // every slot made so far waits for its stream and gives back what it owns
        return rc;
    }
    *out = c;
    return 0;
}

int vx_destroy(vx_ctx* c) {
    if (!c) return 0;
    // The order that must hold (DESIGN.md §6 "Ownership"): the drain unless the
    // context is sticky, the device, every stream waited for, the caller's
    // buffers unregistered (they are not the engine's); only then the members go.
    int rc = c->sticky ? 0 : vx_drain(c, 0);
    set_device(c);
    // A failed (sticky) context skipped the drain: batches may still be
    // running, and a gather kernel may still read registered host memory.
    // Wait for every stream before unregistering anything, so the caller can
    // return in-flight buffers to its pool as soon as this call returns.
    for (auto& s : c->slots)
        if (s.stream) (void)hipStreamSynchronize(s.stream);
    // the re-verify's data copies run on the copy stream: a failed call may
    // have left one queued that still reads a stage or writes an arena
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    // ... and a hybrid slot's merkle work on the side stream reads its arena
    if (c->hy_stream) (void)hipStreamSynchronize(c->hy_stream);
    for (auto& r : c->registered) (void)hipHostUnregister(reinterpret_cast<void*>(r.first));
    // Everything the context owns is a handle member (a new one needs no line
    // here); each stream among them waits once more before it is destroyed.
    delete c;
    return rc;
}

int vx_register_host_buffer(vx_ctx* c, void* ptr, size_t len) {
    if (!c || !ptr || !len) return fail(VX_EINVAL, "vx_register_host_buffer: bad argument");
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
    auto it = c->registered.lower_bound(a);
    if (it != c->registered.end() && it->first < a + len) return fail(VX_EINVAL, "overlapping registration");
    if (it != c->registered.begin()) {
        auto p = std::prev(it);
        if (p->first + p->second.len > a) return fail(VX_EINVAL, "overlapping registration");
    }
    int rc = set_device(c);
    if (rc) return rc;
    VX_HIP(hipHostRegister(ptr, len, hipHostRegisterMapped));
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, ptr, 0) != hipSuccess || !dev) {
        (void)hipHostUnregister(ptr);
        return fail(VX_EDEVICE, "vx_register_host_buffer: no device mapping");
    }
    c->registered[a] = vx_ctx::Reg{len, static_cast<uint8_t*>(dev)};
    c->registered_at[a] = vx_ctx::Reg{len, static_cast<uint8_t*>(dev)};
    return 0;
}

int vx_unregister_host_buffer(vx_ctx* c, void* ptr) {
    if (!c || !ptr) return fail(VX_EINVAL, "vx_unregister_host_buffer: bad argument");
    auto it = c->registered.find(reinterpret_cast<uintptr_t>(ptr));
    if (it == c->registered.end()) return fail(VX_EINVAL, "pointer was not registered");
    if (c->pending) return fail(VX_EBUSY, "unregister with pieces in flight");
    int rc = set_device(c);
    if (rc) return rc;
    VX_HIP(hipHostUnregister(ptr));
    c->registered.erase(it);
    c->registered_at.erase(reinterpret_cast<uintptr_t>(ptr));
    return 0;
}

static int batch_impl(vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, const uint8_t* expected, size_t n,
                      uint8_t* matched_out, uint8_t* digests_out) {
    if (!c) return fail(VX_EINVAL, "batch: NULL context");
    if (n && (!ptrs || !lens)) return fail(VX_EINVAL, "batch: NULL ptrs/lens");
    int rc = begin_bulk_call(c, "batch", /*need_idle=*/false);
    if (!rc) rc = set_device(c);
    if (rc) return rc;
    uint64_t host_stride = 0;
    if (strided_batch(c, ptrs, lens, n, &host_stride))
        return batch_chunked(c, ptrs, lens, expected, n, matched_out, digests_out, host_stride);
    std::vector<const uint8_t*> dev;
    if (gather_batch(c, ptrs, lens, n, dev))
        return batch_chunked_gather(c, lens, expected, n, matched_out, digests_out, dev);
    std::vector<vx_completion> buf(1024);
    size_t got = 0;
    auto collect = [&]() -> int {
        for (;;) {
            int64_t k = vx_poll(c, buf.data(), buf.size());
            if (k < 0) return (int)k;
            for (int64_t j = 0; j < k; ++j) {
                const vx_completion& r = buf[j];
                if (digests_out) std::memcpy(digests_out + r.tag * 20, r.digest, 20);
                if (matched_out) matched_out[r.tag] = r.matched;
            }
            got += (size_t)k;
            if ((size_t)k < buf.size()) return 0;
        }
    };
    // Completions are harvested by acquire_filling when it runs out of slots;
    // polling here between submits would only add event queries to the
    // launch path, so the queue is drained only when it grows large.
    //
    // Pieces go in longest first and each slot fills to its capacity rather
    // than to batch_pieces (which vx_config_default sizes for max_piece_len
    // pieces).  A slot's kernel lasts as long as its longest piece's chain,
    // so in caller order a ragged batch put a long piece into almost every
    // small slot: config 3 from plain host memory ran at 2.1 GiB/s
    // (DESIGN.md §6.4).  Tags stay the caller's indices.
    for (size_t i = 0; i < n; ++i) {  // argument errors before anything is queued
        if (lens[i] > c->cfg.max_piece_len) return fail(VX_ERANGE, "batch: piece longer than max_piece_len");
        if (lens[i] && !ptrs[i]) return fail(VX_EINVAL, "batch: NULL piece pointer");
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return lens[x] > lens[y]; });
    c->bulk = true;
    for (size_t p = 0; p < n; ++p) {
        const size_t i = order[p];
        rc = submit_impl(c, {.kind = Slot::Kind::V1, .tag = i, .data = ptrs[i], .len = lens[i],
                             .expected = expected ? expected + i * 20 : nullptr});
        if (!rc && c->done.size() >= 65536) rc = collect();
        if (rc) break;
    }
    c->bulk = false;
    if (!rc) rc = vx_drain(c, 0);
    if (!rc) rc = collect();
    if (!rc && got != n) rc = fail(VX_EDEVICE, "batch: lost completions");
    if (rc) abandon_batch(c);
    return rc;
}

int vx_sha1_batch(vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, size_t n, uint8_t* digests_out) {
    if (!digests_out && n) return fail(VX_EINVAL, "vx_sha1_batch: NULL digests_out");
    return batch_impl(c, ptrs, lens, nullptr, n, nullptr, digests_out);
}

int vx_verify_batch(vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, const uint8_t* expected, size_t n,
                    uint8_t* matched_out, uint8_t* digests_out) {
    if (n && (!expected || !matched_out)) return fail(VX_EINVAL, "vx_verify_batch: NULL expected/matched_out");
    return batch_impl(c, ptrs, lens, expected, n, matched_out, digests_out);
}
int vx_sha1_device_uniform_variant(const void* d_base, uint64_t stride, uint32_t len, uint32_t n, void* d_digests,
                                   const void* d_expected, void* d_matched, void* stream, int variant) {
    if (n == 0) return 0;
    if (!d_base) return fail(VX_EINVAL, "vx_sha1_device_uniform: NULL base");
    if (!d_digests && !(d_expected && d_matched))
        return fail(VX_EINVAL, "vx_sha1_device_uniform: need d_digests or d_expected+d_matched");
    if (d_matched && !d_expected) return fail(VX_EINVAL, "vx_sha1_device_uniform: d_matched needs d_expected");
    if ((reinterpret_cast<uintptr_t>(d_base) & 15) || (stride & 15))
        return fail(VX_EINVAL, "vx_sha1_device_uniform: base and stride must be 16-byte aligned");
    if (n > 1 && stride < len) return fail(VX_EINVAL, "vx_sha1_device_uniform: stride < len");
    if (variant < 0 || variant > 4)
        return fail(VX_EINVAL, "vx_sha1_device_uniform: unknown variant");
    hipError_t e = vx::launch_uniform(static_cast<const uint8_t*>(d_base), stride, len, n,
                                      static_cast<uint8_t*>(d_digests), static_cast<const uint8_t*>(d_expected),
                                      static_cast<uint8_t*>(d_matched), static_cast<hipStream_t>(stream), variant);
    if (e != hipSuccess) return hip_fail(e, "sha1 uniform kernel launch");
    return 0;
}

int vx_sha1_device_uniform(const void* d_base, uint64_t stride, uint32_t len, uint32_t n, void* d_digests,
                           const void* d_expected, void* d_matched, void* stream) {
    return vx_sha1_device_uniform_variant(d_base, stride, len, n, d_digests, d_expected, d_matched, stream, 0);
}

int vx_sha1_device_ragged_variant(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                                  const uint32_t* d_order, uint32_t n, void* d_digests, const void* d_expected,
                                  void* d_matched, void* stream, int variant) {
    if (n == 0) return 0;
    if (!d_base || !d_offsets || !d_lens) return fail(VX_EINVAL, "vx_sha1_device_ragged: NULL argument");
    if (!d_digests && !(d_expected && d_matched))
        return fail(VX_EINVAL, "vx_sha1_device_ragged: need d_digests or d_expected+d_matched");
    if (d_matched && !d_expected) return fail(VX_EINVAL, "vx_sha1_device_ragged: d_matched needs d_expected");
    if (reinterpret_cast<uintptr_t>(d_base) & 15)
        return fail(VX_EINVAL, "vx_sha1_device_ragged: base must be 16-byte aligned");
    if (variant < 0 || variant > vx::kSplitWide) return fail(VX_EINVAL, "vx_sha1_device_ragged: unknown variant");
    hipError_t e = vx::launch_ragged(static_cast<const uint8_t*>(d_base), d_offsets, d_lens, d_order, n,
                                     static_cast<uint8_t*>(d_digests), static_cast<const uint8_t*>(d_expected),
                                     static_cast<uint8_t*>(d_matched), static_cast<hipStream_t>(stream), variant);
    if (e != hipSuccess) return hip_fail(e, "sha1 ragged kernel launch");
    return 0;
}

int vx_sha1_device_ragged(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                          const uint32_t* d_order, uint32_t n, void* d_digests, const void* d_expected,
                          void* d_matched, void* stream) {
    return vx_sha1_device_ragged_variant(d_base, d_offsets, d_lens, d_order, n, d_digests, d_expected, d_matched,
                                         stream, 0);
}

int vx_sha1_device_ragged_hint(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                               const uint32_t* d_order, uint32_t n, uint32_t max_len, uint64_t total_len,
                               void* d_digests, const void* d_expected, void* d_matched, void* stream) {
    return vx_sha1_device_ragged_variant(d_base, d_offsets, d_lens, d_order, n, d_digests, d_expected, d_matched,
                                         stream, vx::plan_ragged(n, max_len, total_len));
}

int vx_get_stats(const vx_ctx* c, vx_stats* out) {
    if (!c || !out) return fail(VX_EINVAL, "vx_get_stats: NULL argument");
    *out = c->stats;
    return 0;
}

int vx_reset_stats(vx_ctx* c) {
    if (!c) return fail(VX_EINVAL, "vx_reset_stats: NULL context");
    c->stats = vx_stats{};
    return 0;
}

int vx_tuning_zero_copy_plan(uint32_t n, uint64_t total_len) {
    (void)total_len;  // the policy no longer depends on the slot's bytes (kept in the signature)
    return zc_loader_wins(n) ? 2 : 1;
}

int vx_tuning_zero_copy_kernel(const uint64_t* d_srcs, const uint32_t* d_lens, uint32_t n, void* d_digests,
                               const void* d_expected, void* d_matched, int loader, void* stream) {
    if (n && (!d_srcs || !d_lens || !d_digests)) return fail(VX_EINVAL, "vx_tuning_zero_copy_kernel: NULL argument");
    if ((d_expected == nullptr) != (d_matched == nullptr))
        return fail(VX_EINVAL, "vx_tuning_zero_copy_kernel: expected and matched go together");
    hipError_t e = vx::launch_zero_copy(d_srcs, d_lens, n, static_cast<uint8_t*>(d_digests),
                                        static_cast<const uint8_t*>(d_expected), static_cast<uint8_t*>(d_matched),
                                        loader != 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_zero_copy_kernel");
}
#ifdef VX_TEST_HOOKS
int vx_tuning_gather_kernel(const uint64_t* d_src, const uint64_t* d_dst_off, const uint32_t* d_lens,
                            const uint32_t* d_tfirst, uint32_t n, uint32_t ntiles, void* d_arena, uint32_t max_grid,
                            void* stream) {
    if (n == 0) return 0;
    if (!d_src || !d_dst_off || !d_lens || !d_tfirst || !d_arena)
        return fail(VX_EINVAL, "vx_tuning_gather_kernel: NULL argument");
    if (((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst_off)) & 7) ||
        ((reinterpret_cast<uintptr_t>(d_lens) | reinterpret_cast<uintptr_t>(d_tfirst)) & 3) ||
        (reinterpret_cast<uintptr_t>(d_arena) & 15))
        return fail(VX_EINVAL, "vx_tuning_gather_kernel: d_src and d_dst_off must be 8-byte, d_lens and d_tfirst "
                               "4-byte and d_arena 16-byte aligned");
    hipError_t e = vx::launch_gather(d_src, d_dst_off, d_lens, d_tfirst, n, ntiles, static_cast<uint8_t*>(d_arena),
                                     static_cast<hipStream_t>(stream), max_grid);
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_gather_kernel");
}
void vx_tuning_fail_submit_after(vx_ctx* c, int64_t k) {
    if (c) c->fail_submit_after = k < 0 ? -1 : k;
}
void vx_tuning_fail_launch_after(vx_ctx* c, int64_t k) {
    if (c) c->fail_launch_after = k < 0 ? -1 : k;
}
void vx_tuning_verify_copy_stream(vx_ctx* c, int mode) {
    if (c) c->verify_copy_stream = mode ? 1 : 0;
}
void vx_tuning_live_resources(uint64_t* out) {
    for (int k = 0; k < 4 && out; ++k) out[k] = (uint64_t)vx_res::backend::g_live[k].load();
}
void vx_tuning_fail_alloc_after(int64_t n) { vx_res::backend::g_fail_alloc_after = n < 0 ? -1 : n; }
void vx_tuning_stage_huge(vx_ctx* c, int on) {
    if (!c) return;
    c->stage_huge = on ? 1 : 0;
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);  // no copy still reads a stage
    for (auto& s : c->slots)  // reallocated on next use (every slot is idle between calls)
        if (s.state == Slot::FREE) s.stage.reset();
}
#endif
int vx_tuning_plan_ragged(uint32_t n, uint32_t max_len, uint64_t total_len) {
    return vx::plan_ragged(n, max_len, total_len);
}

int vx_sort_order(const uint32_t* lens, uint32_t n, uint32_t* order_out) {
    if (n && (!lens || !order_out)) return fail(VX_EINVAL, "vx_sort_order: NULL argument");
    std::iota(order_out, order_out + n, 0u);
    std::stable_sort(order_out, order_out + n, [lens](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
    return 0;
}

int vx_synth_fill(void* d_base, uint64_t stride, uint32_t len, uint32_t n, uint64_t first, uint64_t seed,
                  uint32_t corrupt_every, void* stream) {
    if (n == 0) return 0;
    if (!d_base) return fail(VX_EINVAL, "vx_synth_fill: NULL base");
    if ((reinterpret_cast<uintptr_t>(d_base) & 15) || (stride & 15) || (n > 1 && stride < len))
        return fail(VX_EINVAL, "vx_synth_fill: base/stride must be 16-byte aligned and stride >= len");
    hipError_t e = vx::launch_synth_fill(static_cast<uint8_t*>(d_base), stride, len, n, first, seed, corrupt_every,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "synth launch");
    return 0;
}

}  // extern "C"
