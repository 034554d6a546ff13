// vx_merkle.hip — the BitTorrent v2 merkle entries of vx_hash.h (kernels in
// sha256_kernels.hip): vx_merkle_device_*, _verify_batch, _layers_plan,
// _verify_layers, _verify_proofs; the block checks (_bitmap_words,
// _device_block_check, _check_blocks) and the layer trees (_tree_plan,
// _device_trees, _build_trees, _tree_proof, _tree_layout).  The files calls
// (_verify_files, _hash_files) are in vx_merkle_files.hip.
#include "vx_engine_internal.hpp"

using namespace vxe;

extern "C" {

// SHA-256(a || b) of two 32-byte hashes on the host: what vx_merkle_pad_hash needs.
static void host_sha256_pair(const uint8_t* a, const uint8_t* b, uint8_t* out) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                     0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (int blk = 0; blk < 2; ++blk) {  // the 64 message bytes, then the padding block
        uint32_t w[64] = {};
        if (blk == 0) {
            for (int k = 0; k < 16; ++k) {
                const uint8_t* p = (k < 8 ? a : b) + 4 * (k & 7);
                w[k] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
            }
        } else {
            w[0] = 0x80000000u;
            w[15] = 512;
        }
        for (int t = 16; t < 64; ++t)
            w[t] = w[t - 16] + (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 7] +
                   (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10));
        uint32_t s[8];
        std::copy(h, h + 8, s);
        for (int t = 0; t < 64; ++t) {
            const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) +
                                ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[t] + w[t];
            const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) +
                                ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
            for (int k = 7; k > 0; --k) s[k] = s[k - 1];
            s[4] += t1;
            s[0] = t1 + t2;
        }
        for (int k = 0; k < 8; ++k) h[k] += s[k];
    }
    for (int k = 0; k < 8; ++k) {
        out[4 * k] = (uint8_t)(h[k] >> 24);
        out[4 * k + 1] = (uint8_t)(h[k] >> 16);
        out[4 * k + 2] = (uint8_t)(h[k] >> 8);
        out[4 * k + 3] = (uint8_t)h[k];
    }
}

constexpr uint32_t kMaxPadHeight = 128;

int vx_merkle_pad_hash(uint32_t height, uint8_t* out) {
    if (!out) return fail(VX_EINVAL, "vx_merkle_pad_hash: NULL out");
    if (height > kMaxPadHeight) return fail(VX_EINVAL, "vx_merkle_pad_hash: height > 128");
    uint8_t cur[32] = {};
    for (uint32_t h = 0; h < height; ++h) {
        uint8_t next[32];
        host_sha256_pair(cur, cur, next);
        std::memcpy(cur, next, 32);
    }
    std::memcpy(out, cur, 32);
    return 0;
}

// What both device entries can check on the host.
static int merkle_args(const char* who, const void* d_base, const void* d_leaves, uint32_t n, uint32_t log2_width) {
    const std::string w(who);
    if (!d_base || !d_leaves) return fail(VX_EINVAL, w + ": NULL d_base or d_leaves");
    if (reinterpret_cast<uintptr_t>(d_base) & 15) return fail(VX_EINVAL, w + ": base must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_leaves) & 15) return fail(VX_EINVAL, w + ": d_leaves must be 16-byte aligned");
    if (log2_width > VX_MERKLE_MAX_LOG2_WIDTH) return fail(VX_EINVAL, w + ": log2_width > 17");
    if (((uint64_t)n << log2_width) >> 32) return fail(VX_EINVAL, w + ": n << log2_width does not fit 32 bits");
    return 0;
}

int vx_merkle_device_uniform(const void* d_base, uint64_t stride, uint32_t len, uint32_t last_len, uint32_t n,
                             uint32_t log2_width, void* d_leaves, void* d_roots, const void* d_expected,
                             void* d_matched, void* stream) {
    if (n == 0) return 0;
    int rc = merkle_args("vx_merkle_device_uniform", d_base, d_leaves, n, log2_width);
    if (rc) return rc;
    if (stride & 15) return fail(VX_EINVAL, "vx_merkle_device_uniform: stride must be a multiple of 16");
    if (stride < len) return fail(VX_EINVAL, "vx_merkle_device_uniform: stride < len");
    if (last_len == 0 || last_len > len) return fail(VX_EINVAL, "vx_merkle_device_uniform: last_len outside (0, len]");
    if (len > (uint64_t)VX_MERKLE_BLOCK << log2_width)
        return fail(VX_EINVAL, "vx_merkle_device_uniform: len > 16384 << log2_width");
    if ((reinterpret_cast<uintptr_t>(d_roots) & 15) || (reinterpret_cast<uintptr_t>(d_expected) & 3))
        return fail(VX_EINVAL, "vx_merkle_device_uniform: d_roots must be 16-byte and d_expected 4-byte aligned");
    const bool verdict = d_expected && d_matched;
    hipError_t e = vx::launch_merkle_uniform(static_cast<const uint8_t*>(d_base), stride, len, last_len, n,
                                             log2_width, static_cast<uint8_t*>(d_leaves),
                                             static_cast<uint8_t*>(d_roots),
                                             verdict ? static_cast<const uint8_t*>(d_expected) : nullptr,
                                             verdict ? static_cast<uint8_t*>(d_matched) : nullptr,
                                             static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle uniform kernel launch");
    return 0;
}

int vx_merkle_device_ragged(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint8_t* d_log2w, uint32_t n, uint32_t log2_width, void* d_leaves, void* d_roots,
                            const void* d_expected, void* d_matched, void* stream) {
    if (n == 0) return 0;
    int rc = merkle_args("vx_merkle_device_ragged", d_base, d_leaves, n, log2_width);
    if (rc) return rc;
    if (!d_offsets || !d_lens) return fail(VX_EINVAL, "vx_merkle_device_ragged: NULL d_offsets or d_lens");
    if ((reinterpret_cast<uintptr_t>(d_roots) & 15) || (reinterpret_cast<uintptr_t>(d_expected) & 3))
        return fail(VX_EINVAL, "vx_merkle_device_ragged: d_roots must be 16-byte and d_expected 4-byte aligned");
    const bool verdict = d_expected && d_matched;
    hipError_t e = vx::launch_merkle_ragged(static_cast<const uint8_t*>(d_base), d_offsets, d_lens, d_log2w, n,
                                            log2_width, static_cast<uint8_t*>(d_leaves),
                                            static_cast<uint8_t*>(d_roots),
                                            verdict ? static_cast<const uint8_t*>(d_expected) : nullptr,
                                            verdict ? static_cast<uint8_t*>(d_matched) : nullptr,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle ragged kernel launch");
    return 0;
}

int vx_merkle_device_pieces(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const uint8_t* d_log2w, uint32_t n, uint32_t log2_width, void* d_work, void* d_roots,
                            const void* d_expected, void* d_matched, void* stream) {
    if (n == 0) return 0;
    // (d_base stands in for the leaf array merkle_args also checks: this entry has none)
    int rc = merkle_args("vx_merkle_device_pieces", d_base, d_base, n, log2_width);
    if (rc) return rc;
    if (!d_offsets || !d_lens) return fail(VX_EINVAL, "vx_merkle_device_pieces: NULL d_offsets or d_lens");
    if ((reinterpret_cast<uintptr_t>(d_roots) & 15) || (reinterpret_cast<uintptr_t>(d_expected) & 3))
        return fail(VX_EINVAL, "vx_merkle_device_pieces: d_roots must be 16-byte and d_expected 4-byte aligned");
    if (log2_width > 8 && (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15)))
        return fail(VX_EINVAL, "vx_merkle_device_pieces: log2_width > 8 needs a 16-byte aligned d_work");
    const bool verdict = d_expected && d_matched;
    hipError_t e = vx::launch_merkle_pieces(static_cast<const uint8_t*>(d_base), d_offsets, d_lens, d_log2w, n,
                                            log2_width, static_cast<uint8_t*>(d_work),
                                            static_cast<uint8_t*>(d_roots),
                                            verdict ? static_cast<const uint8_t*>(d_expected) : nullptr,
                                            verdict ? static_cast<uint8_t*>(d_matched) : nullptr,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle piece kernel launch");
    return 0;
}

int vx_merkle_device_root(const void* d_layer, uint32_t n, uint32_t height, void* d_work, void* d_root,
                          void* stream) {
    if (n == 0) return 0;
    if (!d_layer || !d_root || (n > 1 && !d_work)) return fail(VX_EINVAL, "vx_merkle_device_root: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_layer) | reinterpret_cast<uintptr_t>(d_work) |
         reinterpret_cast<uintptr_t>(d_root)) & 15)
        return fail(VX_EINVAL, "vx_merkle_device_root: buffers must be 16-byte aligned");
    if (height > 64) return fail(VX_EINVAL, "vx_merkle_device_root: height > 64");
    uint8_t pads[33][32];  // pad(height + k), one per level up to the root of 2^32 rows
    vx_merkle_pad_hash(height, pads[0]);
    for (int k = 1; k < 33; ++k) host_sha256_pair(pads[k - 1], pads[k - 1], pads[k]);
    hipError_t e = vx::launch_merkle_root(static_cast<const uint8_t*>(d_layer), n, static_cast<uint8_t*>(d_work),
                                          static_cast<uint8_t*>(d_root), pads, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle layer kernel launch");
    return 0;
}

// Per-slot buffers of vx_merkle_verify_batch.  A round of m pieces packs its
// metadata as expected (32m) | offsets (8m) | lens (4m) | log2w (m) and its
// results as roots (32m) | verdicts (m), so each goes in one copy.
static int ensure_merkle(vx_ctx* c) {
    if (!c->merkle.empty()) return 0;
    const uint64_t rows = align_up(c->slots[0].arena_cap / VX_MERKLE_BLOCK, 16);
    std::vector<vx_ctx::MerkleBufs> bufs(c->slots.size());  // all of them, or (an early return) none
    for (auto& m : bufs)
        if (!m.d.reserve(rows * (48 + 48 + 32)) || !m.h.reserve(rows * (48 + 48)))
            return fail(VX_ENOMEM, "vx_merkle_verify_batch: buffer allocation failed");
    c->merkle = std::move(bufs);
    c->merkle_rows = (uint32_t)rows;
    return 0;
}

int vx_merkle_verify_batch(vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, const uint8_t* log2w,
                           size_t n, uint32_t piece_length, const uint8_t* expected, uint8_t* matched_out,
                           uint8_t* roots_out) {
    if (!c) return fail(VX_EINVAL, "vx_merkle_verify_batch: NULL context");
    if (n && (!ptrs || !lens || !expected || !matched_out))
        return fail(VX_EINVAL, "vx_merkle_verify_batch: NULL ptrs/lens/expected/matched_out");
    if (piece_length < VX_MERKLE_BLOCK || (piece_length & (piece_length - 1)))
        return fail(VX_EINVAL, "vx_merkle_verify_batch: piece_length must be a power of two >= 16384");
    if (piece_length > c->cfg.max_piece_len)
        return fail(VX_ERANGE, "vx_merkle_verify_batch: piece_length > max_piece_len");
    uint32_t log2_width = 0;
    while (((uint32_t)VX_MERKLE_BLOCK << log2_width) < piece_length) ++log2_width;
    for (size_t i = 0; i < n; ++i) {  // argument errors before anything is queued
        const uint32_t lw = log2w ? log2w[i] : log2_width;
        if (lw > log2_width) return fail(VX_EINVAL, "vx_merkle_verify_batch: log2w[i] wider than piece_length");
        if (lens[i] > (uint64_t)VX_MERKLE_BLOCK << lw)
            return fail(VX_EINVAL, "vx_merkle_verify_batch: piece longer than its tree (16384 << log2w[i])");
        if (lens[i] && !ptrs[i]) return fail(VX_EINVAL, "vx_merkle_verify_batch: NULL piece pointer");
    }
    int rc = begin_bulk_call(c, "vx_merkle_verify_batch", /*need_idle=*/true);
    if (rc) return rc;
    if (n == 0) return 0;
    rc = set_device(c);
    if (!rc) rc = ensure_merkle(c);
    if (rc) return rc;

    const size_t nslots = c->slots.size();
    const uint32_t max_pieces = c->merkle_rows >> log2_width;  // >= 1: slot_bytes >= max_piece_len >= piece_length
    struct Round {
        size_t first = 0;
        uint32_t m = 0;
        bool live = false;
    };
    std::vector<Round> rounds(nslots);
    uint64_t n_bad = 0, n_bytes = 0, n_rounds = 0;
    // Wait for the round slot si carries and take its results.
    auto harvest_round = [&](size_t si) -> int {
        Round& r = rounds[si];
        if (!r.live) return 0;
        r.live = false;
        VX_HIP(hipEventSynchronize(c->slots[si].done));
        const uint8_t* out = c->merkle[si].h.get() + (size_t)c->merkle_rows * 48;
        if (roots_out) std::memcpy(roots_out + r.first * 32, out, (size_t)r.m * 32);
        std::memcpy(matched_out + r.first, out + (size_t)r.m * 32, r.m);
        for (uint32_t k = 0; k < r.m; ++k) n_bad += matched_out[r.first + k] == 0;
        return 0;
    };
    size_t next = 0;
    for (size_t k = 0; next < n && !rc; ++k) {
        const size_t si = k % nslots;
        Slot& s = c->slots[si];
        rc = harvest_round(si);  // the slot's last round: its stage and buffers are free again
        if (rc) break;
        const uint64_t R = c->merkle_rows;
        uint8_t* h_in = c->merkle[si].h.get();
        uint8_t* d_in = c->merkle[si].d.get();
        uint8_t* d_out = d_in + R * 48;
        uint8_t* d_leaves = d_in + R * 96;
        // the pieces of this round: as many as the arena and the leaf rows hold
        uint32_t m = 0;
        uint64_t bytes = 0;
        while (next + m < n && m < max_pieces && bytes + align_up(lens[next + m], kAlign) <= s.arena_cap)
            bytes += align_up(lens[next + m++], kAlign);
        if (m == 0) {
            rc = fail(VX_ERANGE, "vx_merkle_verify_batch: a piece does not fit a slot");
            break;
        }
        uint64_t* offs = reinterpret_cast<uint64_t*>(h_in + (size_t)m * 32);
        uint32_t* hl = reinterpret_cast<uint32_t*>(h_in + (size_t)m * 40);
        uint8_t* hw = h_in + (size_t)m * 44;
        std::memcpy(h_in, expected + next * 32, (size_t)m * 32);
        // Plain memory goes through the pinned stage, consecutive pieces in one
        // copy; a registered piece is pinned already and is copied from where it lies.
        uint64_t at = 0, run_lo = 0;
        bool in_run = false;
        auto flush_run = [&](uint64_t hi) -> int {
            if (in_run && hi > run_lo)
                VX_HIP(hipMemcpyAsync(s.d_arena.get() + run_lo, s.stage.get() + run_lo, hi - run_lo, hipMemcpyHostToDevice,
                                      s.stream));
            in_run = false;
            return 0;
        };
        for (uint32_t j = 0; j < m && !rc; ++j) {
            const size_t i = next + j;
            offs[j] = at;
            hl[j] = lens[i];
            hw[j] = log2w ? log2w[i] : (uint8_t)log2_width;
            if (lens[i] && is_registered(c, ptrs[i], lens[i])) {
                rc = flush_run(at);
                if (!rc && hipMemcpyAsync(s.d_arena.get() + at, ptrs[i], lens[i], hipMemcpyHostToDevice, s.stream) !=
                               hipSuccess)
                    rc = fail(VX_EDEVICE, "vx_merkle_verify_batch: copy from registered memory failed");
            } else if (lens[i]) {
                rc = ensure_stage(c, s);
                if (rc) break;
                if (!in_run) {
                    in_run = true;
                    run_lo = at;
                }
                std::memcpy(s.stage.get() + at, ptrs[i], lens[i]);
                c->stats.staged_bytes += lens[i];
            }
            at += align_up(lens[i], kAlign);
            n_bytes += lens[i];
        }
        if (!rc) rc = flush_run(at);
        if (rc) break;
        hipError_t e = hipMemcpyAsync(d_in, h_in, (size_t)m * 45, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess)
            e = vx::launch_merkle_ragged(s.d_arena.get(), reinterpret_cast<const uint64_t*>(d_in + (size_t)m * 32),
                                                reinterpret_cast<const uint32_t*>(d_in + (size_t)m * 40),
                                                d_in + (size_t)m * 44, m, log2_width, d_leaves, d_out, d_in,
                                                d_out + (size_t)m * 32, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_in + R * 48, d_out, (size_t)m * 33, hipMemcpyDeviceToHost, s.stream);
        if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
        if (e != hipSuccess) {
            rc = hip_fail(e, "vx_merkle_verify_batch: enqueue");
            break;
        }
        rounds[si] = Round{next, m, true};
        next += m;
        ++n_rounds;
    }
    // Take what is left in launch order; after an error only wait, so no copy
    // still reads a stage or the caller's registered memory when this returns.
    for (size_t si = 0; si < nslots; ++si) {
        if (!rc) {
            rc = harvest_round(si);
        } else if (c->slots[si].stream) {
            (void)hipStreamSynchronize(c->slots[si].stream);
        }
    }
    if (rc) return rc;
    c->stats.pieces_completed += n;
    c->stats.pieces_mismatched += n_bad;
    c->stats.bytes_completed += n_bytes;
    c->stats.batches += n_rounds;
    return 0;
}

int vx_merkle_device_blocks(const void* d_stage, const uint32_t* d_rows, const uint32_t* d_lens, uint32_t n_blocks,
                            void* d_leaves, void* stream) {
    if (n_blocks == 0) return 0;
    if (!d_stage || !d_rows || !d_lens || !d_leaves) return fail(VX_EINVAL, "vx_merkle_device_blocks: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_stage) | reinterpret_cast<uintptr_t>(d_leaves)) & 15)
        return fail(VX_EINVAL, "vx_merkle_device_blocks: d_stage and d_leaves must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_lens)) & 3)
        return fail(VX_EINVAL, "vx_merkle_device_blocks: d_rows and d_lens must be 4-byte aligned");
    hipError_t e = vx::launch_merkle_blocks(static_cast<const uint8_t*>(d_stage), d_rows, d_lens, n_blocks,
                                            static_cast<uint8_t*>(d_leaves), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle block kernel launch");
    return 0;
}

int vx_merkle_device_nodes(const void* d_leaves, const uint8_t* d_log2w, uint32_t n, uint32_t log2_width,
                           void* d_roots, const void* d_expected, void* d_matched, void* stream) {
    if (n == 0) return 0;
    int rc = merkle_args("vx_merkle_device_nodes", d_leaves, d_leaves, n, log2_width);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(d_roots) & 15) || (reinterpret_cast<uintptr_t>(d_expected) & 3))
        return fail(VX_EINVAL, "vx_merkle_device_nodes: d_roots must be 16-byte and d_expected 4-byte aligned");
    const bool verdict = d_expected && d_matched;
    hipError_t e = vx::launch_merkle_nodes(static_cast<const uint8_t*>(d_leaves), d_log2w, n, log2_width,
                                           static_cast<uint8_t*>(d_roots),
                                           verdict ? static_cast<const uint8_t*>(d_expected) : nullptr,
                                           verdict ? static_cast<uint8_t*>(d_matched) : nullptr,
                                           static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle node kernel launch");
    return 0;
}

int vx_merkle_device_zero_leaves(const uint32_t* d_lens, uint32_t n, void* d_leaves, void* stream) {
    if (n == 0) return 0;
    if (!d_lens || !d_leaves) return fail(VX_EINVAL, "vx_merkle_device_zero_leaves: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_lens) & 3) || (reinterpret_cast<uintptr_t>(d_leaves) & 15))
        return fail(VX_EINVAL, "vx_merkle_device_zero_leaves: d_lens must be 4-byte and d_leaves 16-byte aligned");
    hipError_t e = vx::launch_merkle_zero_leaves(nullptr, d_lens, n, static_cast<uint8_t*>(d_leaves), nullptr,
                                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle zero leaf kernel launch");
    return 0;
}

int vx_tuning_zero_leaf_kernel(const uint32_t* d_rows, const uint32_t* d_lens, uint32_t n, void* d_leaves,
                               const void* full_row, void* stream) {
    if (n == 0) return 0;
    if (!d_lens || !d_leaves) return fail(VX_EINVAL, "vx_tuning_zero_leaf_kernel: NULL argument");
    if (((reinterpret_cast<uintptr_t>(d_lens) | reinterpret_cast<uintptr_t>(d_rows)) & 3) ||
        (reinterpret_cast<uintptr_t>(d_leaves) & 15))
        return fail(VX_EINVAL,
                    "vx_tuning_zero_leaf_kernel: d_rows and d_lens must be 4-byte and d_leaves 16-byte aligned");
    hipError_t e = vx::launch_merkle_zero_leaves(d_rows, d_lens, n, static_cast<uint8_t*>(d_leaves),
                                                 static_cast<const uint8_t*>(full_row),
                                                 static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_zero_leaf_kernel");
}

void vx_tuning_merkle_zc_geometry(uint32_t* out) {
    if (out) vx::merkle_zc_geometry(out);
}

// The launch and, above 256 leaves, the node pass, and nothing else.  The tile
// tops are one process-wide device block, grown on demand and kept: a call
// that grows it waits for the device first, so calls on different streams must
// not overlap at widths above 8.
int vx_tuning_merkle_zc_kernel(const uint64_t* d_srcs, const uint32_t* d_lens, const uint8_t* d_log2w, uint32_t n,
                               uint32_t log2_width, void* d_roots, const void* d_expected, void* d_matched,
                               void* stream) {
    if (n == 0) return 0;
    if (!d_srcs || !d_lens) return fail(VX_EINVAL, "vx_tuning_merkle_zc_kernel: NULL d_srcs or d_lens");
    if ((reinterpret_cast<uintptr_t>(d_srcs) & 7) || (reinterpret_cast<uintptr_t>(d_lens) & 3))
        return fail(VX_EINVAL, "vx_tuning_merkle_zc_kernel: d_srcs must be 8-byte and d_lens 4-byte aligned");
    if (log2_width > VX_MERKLE_MAX_LOG2_WIDTH) return fail(VX_EINVAL, "vx_tuning_merkle_zc_kernel: log2_width > 17");
    if (((uint64_t)n << log2_width) >> 31)
        return fail(VX_EINVAL, "vx_tuning_merkle_zc_kernel: n << log2_width does not fit 31 bits");
    if ((reinterpret_cast<uintptr_t>(d_roots) & 15) || (reinterpret_cast<uintptr_t>(d_expected) & 3))
        return fail(VX_EINVAL, "vx_tuning_merkle_zc_kernel: d_roots must be 16-byte and d_expected 4-byte aligned");
    static std::mutex mu;
    static uint8_t* tops = nullptr;
    static uint64_t tops_cap = 0;
    std::lock_guard<std::mutex> lock(mu);
    const uint64_t need = vx::merkle_pieces_work(n, log2_width);
    if (need > tops_cap) {
        hipError_t e = hipDeviceSynchronize();  // nothing enqueued earlier still writes the old block
        if (e == hipSuccess && tops) e = hipFree(tops);
        tops = nullptr;
        tops_cap = 0;
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&tops), need);
        if (e != hipSuccess) return hip_fail(e, "vx_tuning_merkle_zc_kernel: tile tops allocation");
        tops_cap = need;
    }
    const bool verdict = d_expected && d_matched;
    hipError_t e = vx::launch_merkle_zc_pieces(d_srcs, d_lens, d_log2w, n, log2_width, tops,
                                               static_cast<uint8_t*>(d_roots),
                                               verdict ? static_cast<const uint8_t*>(d_expected) : nullptr,
                                               verdict ? static_cast<uint8_t*>(d_matched) : nullptr,
                                               static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "vx_tuning_merkle_zc_kernel");
}

// ---- `piece layers` and hash proofs in batches ----

int vx_merkle_layers_plan(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_layers_plan* plan,
                          vx_merkle_tile* tiles, size_t tiles_cap) {
    if (!plan || (n_layers && !counts)) return fail(VX_EINVAL, "vx_merkle_layers_plan: NULL plan or counts");
    struct vx_merkle_layers_plan pl;
    if (vx_merkle::plan_layers(counts, n_layers, &pl, nullptr, 0))
        return fail(VX_EINVAL, "vx_merkle_layers_plan: a count is 0, or the counts sum to 2^32 rows or more");
    if (tiles && tiles_cap < pl.n_tiles) return fail(VX_EINVAL, "vx_merkle_layers_plan: tiles_cap < n_tiles");
    return vx_merkle::plan_layers(counts, n_layers, plan, tiles, tiles_cap);
}

int vx_merkle_device_layers(const void* d_hashes, const struct vx_merkle_layers_plan* plan,
                            const vx_merkle_tile* d_tiles, uint32_t height, void* d_work, void* d_roots,
                            const void* d_expected, void* d_matched, void* stream) {
    if (!plan) return fail(VX_EINVAL, "vx_merkle_device_layers: NULL plan");
    if (plan->n_layers == 0) return 0;
    if (!d_hashes || !d_tiles || (plan->work_rows && !d_work))
        return fail(VX_EINVAL, "vx_merkle_device_layers: NULL d_hashes, d_tiles or d_work");
    if ((reinterpret_cast<uintptr_t>(d_hashes) | reinterpret_cast<uintptr_t>(d_work) |
         reinterpret_cast<uintptr_t>(d_roots)) & 15)
        return fail(VX_EINVAL, "vx_merkle_device_layers: d_hashes, d_work and d_roots must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_tiles) | reinterpret_cast<uintptr_t>(d_expected)) & 3)
        return fail(VX_EINVAL, "vx_merkle_device_layers: d_tiles and d_expected must be 4-byte aligned");
    if (height > 64) return fail(VX_EINVAL, "vx_merkle_device_layers: height > 64");
    uint64_t tiles = 0;
    for (uint32_t p = 0; p < 4; ++p) tiles += p < plan->passes ? plan->pass_tiles[p] : 0;
    if (plan->passes > 4 || tiles != plan->n_tiles)
        return fail(VX_EINVAL, "vx_merkle_device_layers: not a plan of vx_merkle_layers_plan (passes, pass_tiles)");
    uint8_t pads[4][32];  // pad(height + 9p), one per pass
    for (int p = 0; p < 4; ++p) vx_merkle_pad_hash(height + 9 * p, pads[p]);
    const bool verdict = d_expected && d_matched;
    hipError_t e = vx::launch_merkle_layers(static_cast<const uint8_t*>(d_hashes), *plan, d_tiles,
                                            static_cast<uint8_t*>(d_work), static_cast<uint8_t*>(d_roots),
                                            verdict ? static_cast<const uint8_t*>(d_expected) : nullptr,
                                            verdict ? static_cast<uint8_t*>(d_matched) : nullptr, pads,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle layers kernel launch");
    return 0;
}

int vx_merkle_device_proofs(const void* d_hashes, const vx_merkle_proof* d_proofs, uint32_t n, void* d_tops,
                            const void* d_expected, void* d_matched, void* stream) {
    if (n == 0) return 0;
    if (!d_hashes || !d_proofs || !d_tops || !d_expected || !d_matched)
        return fail(VX_EINVAL, "vx_merkle_device_proofs: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_hashes) | reinterpret_cast<uintptr_t>(d_tops)) & 15)
        return fail(VX_EINVAL, "vx_merkle_device_proofs: d_hashes and d_tops must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_proofs) & 7) || (reinterpret_cast<uintptr_t>(d_expected) & 3))
        return fail(VX_EINVAL, "vx_merkle_device_proofs: d_proofs must be 8-byte and d_expected 4-byte aligned");
    hipError_t e = vx::launch_merkle_proofs(static_cast<const uint8_t*>(d_hashes), d_proofs, n,
                                            static_cast<uint8_t*>(d_tops), static_cast<const uint8_t*>(d_expected),
                                            static_cast<uint8_t*>(d_matched), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle proof kernel launch");
    return 0;
}

namespace {
// The stream and the one device block of a vx_merkle_verify_layers / _proofs
// call: made per call, gone when it returns (once per torrent or per batch of
// messages; the batch slots and their streams stay with the pieces).
struct CallBufs {
    DeviceMem mem;
    uint8_t* d = nullptr;  // mem's bytes
    // After the block, so gone first and waited for: on an error path no copy
    // may still use the block or the caller's memory.
    Stream stream;
    int make(const vx_ctx* c, uint64_t bytes, const char* who) {
        int rc = set_device(c);
        if (rc) return rc;
        if (!mem.reserve(bytes)) return fail(VX_ENOMEM, std::string(who) + ": buffer allocation failed");
        d = mem.get();
        if (!stream.make(hipStreamNonBlocking)) return fail(VX_EDEVICE, std::string(who) + ": stream creation failed");
        return 0;
    }
};
}  // namespace

int vx_merkle_verify_layers(vx_ctx* c, const uint8_t* hashes, const uint32_t* counts, uint32_t n_layers,
                            uint32_t height, const uint8_t* expected, uint8_t* matched_out, uint8_t* roots_out) {
    const char* who = "vx_merkle_verify_layers";
    if (!c) return fail(VX_EINVAL, std::string(who) + ": NULL context");
    if (n_layers && (!hashes || !counts || !expected || !matched_out))
        return fail(VX_EINVAL, std::string(who) + ": NULL hashes/counts/expected/matched_out");
    if (height > 64) return fail(VX_EINVAL, std::string(who) + ": height > 64");
    if (n_layers == 0) return 0;
    struct vx_merkle_layers_plan plan;
    if (vx_merkle::plan_layers(counts, n_layers, &plan, nullptr, 0))
        return fail(VX_EINVAL, std::string(who) + ": a count is 0, or the counts sum to 2^32 rows or more");
    if (c->sticky) return c->sticky;
    std::vector<vx_merkle_tile> tiles(plan.n_tiles);
    (void)vx_merkle::plan_layers(counts, n_layers, &plan, tiles.data(), tiles.size());
    // hashes | work | roots | expected | tiles | verdicts: every part but the last a multiple of 16 bytes
    const uint64_t o_work = plan.rows * 32, o_roots = o_work + plan.work_rows * 32;
    const uint64_t o_exp = o_roots + (uint64_t)n_layers * 32, o_tiles = o_exp + (uint64_t)n_layers * 32;
    const uint64_t o_match = o_tiles + (uint64_t)plan.n_tiles * sizeof(vx_merkle_tile);
    CallBufs b;
    int rc = b.make(c, o_match + n_layers, who);
    if (rc) return rc;
    VX_HIP(hipMemcpyAsync(b.d, hashes, plan.rows * 32, hipMemcpyHostToDevice, b.stream));
    VX_HIP(hipMemcpyAsync(b.d + o_exp, expected, (size_t)n_layers * 32, hipMemcpyHostToDevice, b.stream));
    VX_HIP(hipMemcpyAsync(b.d + o_tiles, tiles.data(), tiles.size() * sizeof(vx_merkle_tile), hipMemcpyHostToDevice,
                          b.stream));
    rc = vx_merkle_device_layers(b.d, &plan, reinterpret_cast<const vx_merkle_tile*>(b.d + o_tiles), height,
                                 b.d + o_work, b.d + o_roots, b.d + o_exp, b.d + o_match, b.stream);
    if (rc) return rc;
    if (roots_out) VX_HIP(hipMemcpyAsync(roots_out, b.d + o_roots, (size_t)n_layers * 32, hipMemcpyDeviceToHost, b.stream));
    VX_HIP(hipMemcpyAsync(matched_out, b.d + o_match, n_layers, hipMemcpyDeviceToHost, b.stream));
    VX_HIP(hipStreamSynchronize(b.stream));
    return 0;
}

int vx_merkle_verify_proofs(vx_ctx* c, const uint8_t* hashes, uint64_t n_rows, const vx_merkle_proof* proofs,
                            uint32_t n, const uint8_t* expected, uint32_t n_expected, uint8_t* matched_out,
                            uint8_t* tops_out) {
    const char* who = "vx_merkle_verify_proofs";
    if (!c) return fail(VX_EINVAL, std::string(who) + ": NULL context");
    if (n && (!hashes || !proofs || !expected || !matched_out))
        return fail(VX_EINVAL, std::string(who) + ": NULL hashes/proofs/expected/matched_out");
    for (uint32_t i = 0; i < n; ++i) {  // wire-derived numbers: checked before anything is copied
        const vx_merkle_proof& p = proofs[i];
        const char* bad = nullptr;
        if (p.span == 0 || p.span > VX_MERKLE_TILE_ROWS || (p.span & (p.span - 1)))
            bad = "span is not a power of two in 1..512";
        else if (p.uncles > 64)
            bad = "uncles > 64";
        else if ((uint64_t)p.row + p.span + p.uncles > n_rows)
            bad = "row + span + uncles > n_rows";
        else if (p.expected >= n_expected)
            bad = "expected >= n_expected";
        if (bad) return fail(VX_EINVAL, std::string(who) + ": proof " + std::to_string(i) + ": " + bad);
    }
    if (n == 0) return 0;
    if (c->sticky) return c->sticky;
    // hashes | tops | expected | proofs | verdicts: every part but the last a multiple of 8 bytes
    const uint64_t o_tops = n_rows * 32, o_exp = o_tops + (uint64_t)n * 32;
    const uint64_t o_proofs = o_exp + (uint64_t)n_expected * 32;
    const uint64_t o_match = o_proofs + (uint64_t)n * sizeof(vx_merkle_proof);
    CallBufs b;
    int rc = b.make(c, o_match + n, who);
    if (rc) return rc;
    VX_HIP(hipMemcpyAsync(b.d, hashes, n_rows * 32, hipMemcpyHostToDevice, b.stream));
    VX_HIP(hipMemcpyAsync(b.d + o_exp, expected, (size_t)n_expected * 32, hipMemcpyHostToDevice, b.stream));
    VX_HIP(hipMemcpyAsync(b.d + o_proofs, proofs, (size_t)n * sizeof(vx_merkle_proof), hipMemcpyHostToDevice,
                          b.stream));
    rc = vx_merkle_device_proofs(b.d, reinterpret_cast<const vx_merkle_proof*>(b.d + o_proofs), n, b.d + o_tops,
                                 b.d + o_exp, b.d + o_match, b.stream);
    if (rc) return rc;
    if (tops_out) VX_HIP(hipMemcpyAsync(tops_out, b.d + o_tops, (size_t)n * 32, hipMemcpyDeviceToHost, b.stream));
    VX_HIP(hipMemcpyAsync(matched_out, b.d + o_match, n, hipMemcpyDeviceToHost, b.stream));
    VX_HIP(hipStreamSynchronize(b.stream));
    return 0;
}

// ---- block checks ("Block checks") ----

uint64_t vx_merkle_bitmap_words(uint32_t n, uint32_t log2_width) {
    if (log2_width > VX_MERKLE_MAX_LOG2_WIDTH) return 0;
    return (uint64_t)n * std::max<uint64_t>(1, (1ull << log2_width) / 64);
}

int vx_merkle_device_block_check(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t n,
                                 uint32_t log2_width, const void* d_expected_leaves, uint64_t* d_bad,
                                 void* d_leaves_out, void* stream) {
    if (n == 0) return 0;
    const char* who = "vx_merkle_device_block_check";
    // (d_base stands in for the leaf array merkle_args also checks when the call keeps none)
    int rc = merkle_args(who, d_base, d_leaves_out ? d_leaves_out : d_base, n, log2_width);
    if (rc) return rc;
    if (!d_offsets || !d_lens) return fail(VX_EINVAL, std::string(who) + ": NULL d_offsets or d_lens");
    if (!d_expected_leaves != !d_bad)
        return fail(VX_EINVAL, std::string(who) + ": d_expected_leaves and d_bad are given together or not at all");
    if (!d_expected_leaves && !d_leaves_out)
        return fail(VX_EINVAL, std::string(who) + ": neither a bitmap nor d_leaves_out asked for");
    if ((reinterpret_cast<uintptr_t>(d_expected_leaves) & 15) || (reinterpret_cast<uintptr_t>(d_bad) & 7))
        return fail(VX_EINVAL, std::string(who) + ": d_expected_leaves must be 16-byte and d_bad 8-byte aligned");
    hipError_t e = vx::launch_merkle_block_check(static_cast<const uint8_t*>(d_base), d_offsets, d_lens, n, log2_width,
                                                 static_cast<const uint8_t*>(d_expected_leaves), d_bad,
                                                 static_cast<uint8_t*>(d_leaves_out), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle block check kernel launch");
    return 0;
}

int vx_merkle_check_blocks(vx_ctx* c, const uint8_t* const* ptrs, const uint32_t* lens, size_t n,
                           uint32_t piece_length, const uint8_t* expected_leaves, uint64_t* bad_out,
                           uint32_t* bad_counts_out, uint8_t* leaves_out) {
    const char* who = "vx_merkle_check_blocks";
    if (!c) return fail(VX_EINVAL, std::string(who) + ": NULL context");
    if (n && (!ptrs || !lens)) return fail(VX_EINVAL, std::string(who) + ": NULL ptrs/lens");
    if (n && !expected_leaves != !bad_out)
        return fail(VX_EINVAL, std::string(who) + ": bad_out is required iff expected_leaves is given");
    if (n && !expected_leaves && bad_counts_out)
        return fail(VX_EINVAL, std::string(who) + ": bad_counts_out needs expected_leaves");
    if (n && !expected_leaves && !leaves_out)
        return fail(VX_EINVAL, std::string(who) + ": neither expected_leaves nor leaves_out given");
    if (piece_length < VX_MERKLE_BLOCK || (piece_length & (piece_length - 1)))
        return fail(VX_EINVAL, std::string(who) + ": piece_length must be a power of two >= 16384");
    if (piece_length > c->cfg.max_piece_len) return fail(VX_ERANGE, std::string(who) + ": piece_length > max_piece_len");
    uint32_t log2_width = 0;
    while (((uint32_t)VX_MERKLE_BLOCK << log2_width) < piece_length) ++log2_width;
    for (size_t i = 0; i < n; ++i) {  // argument errors before anything is allocated or copied
        if (lens[i] > piece_length) return fail(VX_EINVAL, std::string(who) + ": piece longer than piece_length");
        if (lens[i] && !ptrs[i]) return fail(VX_EINVAL, std::string(who) + ": NULL piece pointer");
    }
    if (n == 0) return 0;
    if (c->sticky) return c->sticky;
    // Rounds: as many pieces as slot_bytes of 16-byte aligned piece bytes and
    // slot_bytes / 16 KiB leaf rows hold (one piece at least: piece_length <=
    // max_piece_len <= slot_bytes).  Planned first, so the one device block is
    // sized for the largest of them.
    const uint64_t W = 1ull << log2_width, wpp = std::max<uint64_t>(1, W / 64);
    const uint64_t cap_bytes = c->cfg.slot_bytes;
    const uint64_t cap_pieces = std::max<uint64_t>(1, (cap_bytes / VX_MERKLE_BLOCK) >> log2_width);
    auto round_at = [&](size_t first, uint64_t* bytes_out) -> uint32_t {
        uint32_t m = 0;
        uint64_t bytes = 0;
        while (first + m < n && m < cap_pieces && bytes + align_up(lens[first + m], 16) <= cap_bytes)
            bytes += align_up(lens[first + m++], 16);
        *bytes_out = bytes;
        return m;
    };
    uint64_t max_m = 0, max_bytes = 0;
    for (size_t first = 0; first < n;) {
        uint64_t bytes;
        const uint32_t m = round_at(first, &bytes);
        if (m == 0) return fail(VX_ERANGE, std::string(who) + ": a piece does not fit slot_bytes");
        max_m = std::max<uint64_t>(max_m, m);
        max_bytes = std::max(max_bytes, bytes);
        first += m;
    }
    // arena | expected rows | leaf rows | offsets | bitmap | lens: each part as aligned as it must be
    const uint64_t o_exp = align_up(std::max<uint64_t>(max_bytes, 16), 16);
    const uint64_t o_leaves = o_exp + (expected_leaves ? max_m * W * 32 : 0);
    const uint64_t o_offs = o_leaves + (leaves_out ? max_m * W * 32 : 0);
    const uint64_t o_bad = o_offs + max_m * 8;
    const uint64_t o_lens = o_bad + (expected_leaves ? max_m * wpp * 8 : 0);
    CallBufs b;
    int rc = b.make(c, o_lens + max_m * 4, who);
    if (rc) return rc;
    std::vector<uint64_t> offs(max_m);
    for (size_t first = 0; first < n;) {
        uint64_t bytes;
        const uint32_t m = round_at(first, &bytes);
        uint64_t at = 0;
        for (uint32_t j = 0; j < m; ++j) {
            const size_t i = first + j;
            offs[j] = at;
            if (lens[i]) VX_HIP(hipMemcpyAsync(b.d + at, ptrs[i], lens[i], hipMemcpyHostToDevice, b.stream));
            at += align_up(lens[i], 16);
        }
        const uint64_t rows = (uint64_t)m * W;
        VX_HIP(hipMemcpyAsync(b.d + o_offs, offs.data(), (size_t)m * 8, hipMemcpyHostToDevice, b.stream));
        VX_HIP(hipMemcpyAsync(b.d + o_lens, lens + first, (size_t)m * 4, hipMemcpyHostToDevice, b.stream));
        if (expected_leaves)
            VX_HIP(hipMemcpyAsync(b.d + o_exp, expected_leaves + first * W * 32, rows * 32, hipMemcpyHostToDevice,
                                  b.stream));
        rc = vx_merkle_device_block_check(b.d, reinterpret_cast<const uint64_t*>(b.d + o_offs),
                                          reinterpret_cast<const uint32_t*>(b.d + o_lens), m, log2_width,
                                          expected_leaves ? b.d + o_exp : nullptr,
                                          expected_leaves ? reinterpret_cast<uint64_t*>(b.d + o_bad) : nullptr,
                                          leaves_out ? b.d + o_leaves : nullptr, b.stream);
        if (rc) return rc;
        if (expected_leaves)
            VX_HIP(hipMemcpyAsync(bad_out + first * wpp, b.d + o_bad, (size_t)m * wpp * 8, hipMemcpyDeviceToHost,
                                  b.stream));
        if (leaves_out)
            VX_HIP(hipMemcpyAsync(leaves_out + first * W * 32, b.d + o_leaves, rows * 32, hipMemcpyDeviceToHost,
                                  b.stream));
        VX_HIP(hipStreamSynchronize(b.stream));  // offs and the arena are the next round's
        first += m;
    }
    if (bad_counts_out)
        for (size_t i = 0; i < n; ++i) {
            uint32_t count = 0;
            for (uint64_t k = 0; k < wpp; ++k) count += (uint32_t)__builtin_popcountll(bad_out[i * wpp + k]);
            bad_counts_out[i] = count;
        }
    return 0;
}

// ---- layer trees ("Layer trees") ----

uint64_t vx_merkle_tree_rows(uint64_t m) { return vx_merkle::tree_rows(m); }

int vx_merkle_tree_plan(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_tree_plan* plan,
                        vx_merkle_tree_tile* tiles, size_t tiles_cap, uint64_t* tree_off) {
    if (!plan || (n_layers && !counts)) return fail(VX_EINVAL, "vx_merkle_tree_plan: NULL plan or counts");
    struct vx_merkle_tree_plan pl;
    if (vx_merkle::plan_trees(counts, n_layers, &pl, nullptr, 0, nullptr))
        return fail(VX_EINVAL,
                    "vx_merkle_tree_plan: a count is 0, or the layers or their trees hold 2^32 rows or more");
    if (tiles && tiles_cap < pl.n_tiles) return fail(VX_EINVAL, "vx_merkle_tree_plan: tiles_cap < n_tiles");
    return vx_merkle::plan_trees(counts, n_layers, plan, tiles, tiles_cap, tree_off);
}

int vx_merkle_device_trees(const void* d_hashes, const struct vx_merkle_tree_plan* plan,
                           const vx_merkle_tree_tile* d_tiles, uint32_t height, void* d_tree, void* stream) {
    if (!plan) return fail(VX_EINVAL, "vx_merkle_device_trees: NULL plan");
    if (plan->n_layers == 0) return 0;
    if (!d_hashes || !d_tiles || !d_tree) return fail(VX_EINVAL, "vx_merkle_device_trees: NULL d_hashes, d_tiles or d_tree");
    if ((reinterpret_cast<uintptr_t>(d_hashes) | reinterpret_cast<uintptr_t>(d_tree)) & 15)
        return fail(VX_EINVAL, "vx_merkle_device_trees: d_hashes and d_tree must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_tiles) & 3)
        return fail(VX_EINVAL, "vx_merkle_device_trees: d_tiles must be 4-byte aligned");
    if (height > 64) return fail(VX_EINVAL, "vx_merkle_device_trees: height > 64");
    uint64_t tiles = 0;
    for (uint32_t p = 0; p < 4; ++p) tiles += p < plan->passes ? plan->pass_tiles[p] : 0;
    if (plan->passes > 4 || tiles != plan->n_tiles || (plan->tree_rows >> 32) || plan->tree_rows < plan->rows)
        return fail(VX_EINVAL, "vx_merkle_device_trees: not a plan of vx_merkle_tree_plan (passes, pass_tiles, rows)");
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(d_hashes), t0 = reinterpret_cast<uintptr_t>(d_tree);
    if (h0 < t0 + plan->tree_rows * 32 && t0 < h0 + plan->rows * 32)
        return fail(VX_EINVAL, "vx_merkle_device_trees: d_tree overlaps d_hashes");
    uint8_t pads[4][32];  // pad(height + 9p), one per pass
    for (int p = 0; p < 4; ++p) vx_merkle_pad_hash(height + 9 * p, pads[p]);
    hipError_t e = vx::launch_merkle_trees(static_cast<const uint8_t*>(d_hashes), *plan, d_tiles,
                                           static_cast<uint8_t*>(d_tree), pads, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle tree kernel launch");
    return 0;
}

int vx_merkle_build_trees(vx_ctx* c, const uint8_t* hashes, const uint32_t* counts, uint32_t n_layers,
                          uint32_t height, uint8_t* tree_out, uint8_t* roots_out) {
    const char* who = "vx_merkle_build_trees";
    if (!c) return fail(VX_EINVAL, std::string(who) + ": NULL context");
    if (n_layers && (!hashes || !counts || !tree_out))
        return fail(VX_EINVAL, std::string(who) + ": NULL hashes/counts/tree_out");
    if (height > 64) return fail(VX_EINVAL, std::string(who) + ": height > 64");
    if (n_layers == 0) return 0;
    struct vx_merkle_tree_plan plan;
    if (vx_merkle::plan_trees(counts, n_layers, &plan, nullptr, 0, nullptr))
        return fail(VX_EINVAL, std::string(who) + ": a count is 0, or the layers or their trees hold 2^32 rows or more");
    if (c->sticky) return c->sticky;
    std::vector<vx_merkle_tree_tile> tiles(plan.n_tiles);
    std::vector<uint64_t> off((size_t)n_layers + 1);
    (void)vx_merkle::plan_trees(counts, n_layers, &plan, tiles.data(), tiles.size(), off.data());
    // hashes | tree | tiles: every part a multiple of 16 bytes
    const uint64_t o_tree = plan.rows * 32, o_tiles = o_tree + plan.tree_rows * 32;
    CallBufs b;
    int rc = b.make(c, o_tiles + (uint64_t)plan.n_tiles * sizeof(vx_merkle_tree_tile), who);
    if (rc) return rc;
    VX_HIP(hipMemcpyAsync(b.d, hashes, plan.rows * 32, hipMemcpyHostToDevice, b.stream));
    VX_HIP(hipMemcpyAsync(b.d + o_tiles, tiles.data(), tiles.size() * sizeof(vx_merkle_tree_tile),
                          hipMemcpyHostToDevice, b.stream));
    rc = vx_merkle_device_trees(b.d, &plan, reinterpret_cast<const vx_merkle_tree_tile*>(b.d + o_tiles), height,
                                b.d + o_tree, b.stream);
    if (rc) return rc;
    VX_HIP(hipMemcpyAsync(tree_out, b.d + o_tree, plan.tree_rows * 32, hipMemcpyDeviceToHost, b.stream));
    VX_HIP(hipStreamSynchronize(b.stream));
    if (roots_out)
        for (uint32_t f = 0; f < n_layers; ++f) std::memcpy(roots_out + (size_t)f * 32, tree_out + (off[f + 1] - 1) * 32, 32);
    return 0;
}

int vx_merkle_tree_proof(const uint8_t* tree, uint32_t m, uint32_t height, uint32_t level, uint64_t pos,
                         uint32_t span, uint32_t uncles, uint8_t* out) {
    if (!tree || !out) return fail(VX_EINVAL, "vx_merkle_tree_proof: NULL tree or out");
    // pad(0..): made once, 169 hashes (the lookup itself hashes nothing)
    static const std::vector<uint8_t> pads = [] {
        std::vector<uint8_t> p((size_t)vx_merkle::kProofPads * 32, 0);
        for (uint32_t h = 1; h < vx_merkle::kProofPads; ++h)
            host_sha256_pair(p.data() + (size_t)(h - 1) * 32, p.data() + (size_t)(h - 1) * 32, p.data() + (size_t)h * 32);
        return p;
    }();
    if (vx_merkle::tree_proof(tree, m, height, level, pos, span, uncles, pads.data(), out))
        return fail(VX_EINVAL,
                    "vx_merkle_tree_proof: m == 0, height > 64, span not a power of two in 1..512, uncles > 64, "
                    "level > K, or a span past the level's rows");
    return 0;
}

int64_t vx_merkle_tree_layout(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length,
                              uint32_t* counts_out, uint64_t* tree_off_out) {
    if (nfiles && !file_lengths) return fail(VX_EINVAL, "vx_merkle_tree_layout: NULL file_lengths");
    if (piece_length < VX_MERKLE_BLOCK || (piece_length & (piece_length - 1)))
        return fail(VX_EINVAL, "vx_merkle_tree_layout: piece_length must be a power of two >= 16384");
    const int64_t rows = vx_merkle::tree_layout(file_lengths, nfiles, piece_length, counts_out, tree_off_out);
    if (rows < 0) return fail(VX_EINVAL, "vx_merkle_tree_layout: a file has 2^32 pieces or more");
    return rows;
}

}  // extern "C"
