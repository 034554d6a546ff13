// sha1_tail_kernels.hip — the zero-tail continuation of a hybrid torrent's v1
// pieces, in a unit of its own so the code layout of
// sha1_kernels.hip (§3.6) does not move.
//
// A hybrid (BEP 52 "upgrade path") torrent pads every file but the last to a
// piece boundary with a BEP 47 pad file, so the v1 piece that ends a file is
//   data (data_len bytes) ‖ zeros (pad_len bytes),  data_len + pad_len = piece_length.
// The chunked kernel of sha1_kernels.hip hashes the data_len >> 6 whole data
// blocks and leaves the chaining state; this kernel takes it from there, one
// lane per padded piece:
//   * the one mixed block (the data_len & 63 tail bytes, then zeros; no 0x80),
//     with the general compression, if there are tail bytes;
//   * Z all-zero blocks.  W[t] = 0 for all t, so a round is
//     rotl(a,5) + f(b,c,d) + e + K and rotl(b,30): 5 VALU ops, nothing to
//     load, no schedule and no LDS ring;
//   * the final padding block of a piece_length-byte message.  piece_length is
//     a multiple of 64, so that block (0x80, zeros, the bit length) is the same
//     for every lane of a launch: the host expands its 80 schedule words once,
//     adds the round constants and passes them as a kernel argument, so the
//     final block costs what a zero block costs with K + W[t] in an SGPR.
// The zero-block loop runs to the wave's largest Z; lanes that are done keep
// their state under a select.  Lanes past n, and lanes whose pad_len is 0 (an
// unpadded piece ends in the chunked kernel), store nothing.
//
// The same zero-block round hashes whole zero pieces from nothing
// (sha1_zero_kernel at the end of this file): the digests the
// file re-verify compares unwritten pieces' expected rows with.
#include "sha1_device.hpp"
#include "vx_kernels.h"

namespace vx {

namespace {

constexpr int kTailBlock = 64;  // one wave: a launch of few long chains still spreads over the CUs

// (as in sha1_kernels.hip, whose copies are local to that unit)
__device__ __forceinline__ uint32_t tail_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

__device__ __forceinline__ void tail_emit(const State& s, uint32_t idx, uint8_t* __restrict__ digests,
                                          const uint8_t* __restrict__ expected, uint8_t* __restrict__ matched) {
    const uint32_t d0 = bswap(s.h0), d1 = bswap(s.h1), d2 = bswap(s.h2), d3 = bswap(s.h3), d4 = bswap(s.h4);
    if (digests) {
        uint32_t* o = reinterpret_cast<uint32_t*>(digests + (size_t)idx * 20);
        o[0] = d0;
        o[1] = d1;
        o[2] = d2;
        o[3] = d3;
        o[4] = d4;
    }
    if (expected && matched) {
        const uint32_t* x = reinterpret_cast<const uint32_t*>(expected + (size_t)idx * 20);
        const bool ok = (x[0] == d0) & (x[1] == d1) & (x[2] == d2) & (x[3] == d3) & (x[4] == d4);
        matched[idx] = ok ? 1 : 0;
    }
}

// One block whose 80 schedule words are known: kw(t) = K(t) + W[t].
template <typename KW>
__device__ __forceinline__ void compress_known(State& s, KW kw) {
    uint32_t a = s.h0, b = s.h1, c = s.h2, d = s.h3, e = s.h4;
#pragma unroll
    for (int t = 0; t < 80; ++t) {
        const uint32_t f = t < 20 ? VX_CH(b, c, d) : (t >= 40 && t < 60) ? VX_MAJ(b, c, d) : VX_PAR(b, c, d);
        const uint32_t x = f + e + kw(t);  // off the chain: a is not in it
        const uint32_t tmp = rotl(a, 5) + x;
        e = d;
        d = c;
        c = rotl(b, 30);
        b = a;
        a = tmp;
    }
    s.h0 += a;
    s.h1 += b;
    s.h2 += c;
    s.h3 += d;
    s.h4 += e;
}

struct ZeroWords {
    __device__ __forceinline__ uint32_t operator()(int t) const {
        return t < 20 ? kK0 : t < 40 ? kK1 : t < 60 ? kK2 : kK3;
    }
};

struct FinalWords {
    const TailSched& f;
    __device__ __forceinline__ uint32_t operator()(int t) const { return f.kw[t]; }
};

}  // namespace

__global__ __launch_bounds__(kTailBlock) void sha1_zero_tail_kernel(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ tail_offs, const uint32_t* __restrict__ lens,
    const uint32_t* __restrict__ pads, const uint32_t* __restrict__ pids, uint32_t n,
    const uint32_t* __restrict__ states, uint8_t* __restrict__ digests, const uint8_t* __restrict__ expected,
    uint8_t* __restrict__ matched, const TailSched fin) {
    const uint32_t j = blockIdx.x * kTailBlock + threadIdx.x;
    const uint32_t jj = j < n ? j : n - 1;  // lanes past n redo lane n-1 (in bounds) and store nothing
    const uint32_t len = lens[jj], pad = pads[jj];
    const uint32_t pid = pids ? pids[jj] : jj;
    const bool live = j < n && pad != 0;
    const uint32_t rem = live ? len & 63u : 0u;
    const uint32_t fill = rem ? 64u - rem : 0u;  // zeros that complete the mixed block
    const uint32_t z = live && pad >= fill ? (pad - fill) >> 6 : 0u;
    const uint32_t z_wave = __builtin_amdgcn_readfirstlane(tail_wave_max(z));

    State s = iv();
    if (len >> 6) {
        const uint32_t* st = states + (size_t)pid * 5;
        s = State{st[0], st[1], st[2], st[3], st[4]};
    }
    if (rem) {
        // Only the aligned words that hold a tail byte are loaded (such a word
        // cannot leave the byte's page), and what follows the tail in the
        // last of them is masked off: it is not the piece's.
        const uint32_t* q32 = reinterpret_cast<const uint32_t*>(base + tail_offs[jj]);  // 4-byte aligned
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t off = 4u * k;
            uint32_t v = off < rem ? q32[k] : 0u;
            if (rem - off < 4u) v &= (1u << (8u * (rem - off))) - 1u;  // (rem < off wraps: no mask, v is 0)
            w[k] = bswap(v);
        }
        compress(s, w);
    }
    for (uint32_t b = 0; b < z_wave; ++b) {
        State t = s;
        compress_known(t, ZeroWords{});
        const bool mine = b < z;
        s.h0 = mine ? t.h0 : s.h0;
        s.h1 = mine ? t.h1 : s.h1;
        s.h2 = mine ? t.h2 : s.h2;
        s.h3 = mine ? t.h3 : s.h3;
        s.h4 = mine ? t.h4 : s.h4;
    }
    compress_known(s, FinalWords{fin});
    if (live) tail_emit(s, pid, digests, expected, matched);
}

// A run of zeros in the middle of a piece's chain: a
// chunk of a hybrid piece that the file system never wrote, in front of a chunk
// that it did.  Lane j takes the state row of piece pids[j] (the IV when the
// run starts the piece, poffs[j] == 0: the row is then not read), runs
// blocks[j] zero blocks through the tail kernel's zero-block round (to the
// wave's largest count, lanes that are done keep their state under a select)
// and stores the state back to the same row: no final block, no digest, no
// verdict.  Nothing is loaded but the three table words and the state; lanes
// past n redo lane n - 1 (in bounds) and store nothing.
__global__ __launch_bounds__(kTailBlock) void sha1_zero_run_kernel(const uint32_t* __restrict__ pids,
                                                                   const uint32_t* __restrict__ poffs,
                                                                   const uint32_t* __restrict__ blocks, uint32_t n,
                                                                   uint32_t* __restrict__ states) {
    const uint32_t j = blockIdx.x * kTailBlock + threadIdx.x;
    const uint32_t jj = j < n ? j : n - 1;
    const uint32_t z = blocks[jj];
    const uint32_t z_wave = __builtin_amdgcn_readfirstlane(tail_wave_max(z));
    uint32_t* st = states + (size_t)pids[jj] * 5;

    State s = iv();
    if (poffs[jj] != 0) s = State{st[0], st[1], st[2], st[3], st[4]};
    for (uint32_t b = 0; b < z_wave; ++b) {
        State t = s;
        compress_known(t, ZeroWords{});
        const bool mine = b < z;
        s.h0 = mine ? t.h0 : s.h0;
        s.h1 = mine ? t.h1 : s.h1;
        s.h2 = mine ? t.h2 : s.h2;
        s.h3 = mine ? t.h3 : s.h3;
        s.h4 = mine ? t.h4 : s.h4;
    }
    if (j < n) {
        st[0] = s.h0;
        st[1] = s.h1;
        st[2] = s.h2;
        st[3] = s.h3;
        st[4] = s.h4;
    }
}

// The tables the chunked kernel and the tail kernel take for
// vx_hybrid_device_pieces, from the caller's device-resident lens and pads:
// a padded piece's chunk is its whole 64-byte blocks and is not final (total
// length len + pad), an unpadded piece's chunk is the piece.
__global__ __launch_bounds__(kBlock) void hybrid_prep_kernel(const uint64_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ lens,
                                                             const uint32_t* __restrict__ pads, uint32_t n,
                                                             uint64_t* __restrict__ tail_offs,
                                                             uint64_t* __restrict__ poffs,
                                                             uint64_t* __restrict__ tlens,
                                                             uint32_t* __restrict__ clens,
                                                             uint32_t* __restrict__ pids) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = lens[i], pad = pads[i];
    tail_offs[i] = offsets[i] + (len & ~63u);
    poffs[i] = 0;
    tlens[i] = (uint64_t)len + pad;
    clens[i] = pad ? len & ~63u : len;
    pids[i] = i;
}

// matched[i] = (SHA-1 verdict) | (root verdict) << 1; a NULL side gives a clear bit.
__global__ __launch_bounds__(kBlock) void hybrid_merge_kernel(const uint8_t* __restrict__ v1,
                                                              const uint8_t* __restrict__ v2, uint32_t n,
                                                              uint8_t* __restrict__ matched) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    matched[i] = (uint8_t)((v1 && v1[i] ? 1u : 0u) | (v2 && v2[i] ? 2u : 0u));
}

// The end of a hybrid download slot (vx_hybrid_submit), one
// lane per piece: in place of the tail launch plus hybrid_merge_kernel, and
// the one kernel that compares both hashes with rows named by an index.
//   * A padded lane (pads[j] != 0) continues as sha1_zero_tail_kernel does, from
//     states[5j..] (the IV when the piece has no whole block) through the
//     mixed block, its zero blocks and the launch's final block (every padded
//     piece of a launch has one total length), and writes digest row j.
//   * An unpadded lane's digest row was written by the chunked kernel.
//   * Every lane < n then compares its digest and its root (row j of roots,
//     from the merkle path) with row r of exp_sha1 / exp_roots, r =
//     exp_index[j] or j, and writes matched[j]: bit 0 = SHA-1 equal and
//     flags[j] bit 0, bit 1 = root equal and flags[j] bit 1.  A side whose
//     flag bit is clear is not read.
// A wave with no padded lane skips the SHA-1 part.  Lanes past n redo lane
// n - 1 (in bounds) and store nothing.
__global__ __launch_bounds__(kTailBlock) void hybrid_finish_kernel(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ tail_offs, const uint32_t* __restrict__ lens,
    const uint32_t* __restrict__ pads, uint32_t n, const uint32_t* __restrict__ states, uint8_t* digests,
    const uint8_t* __restrict__ roots, const uint8_t* __restrict__ exp_sha1, const uint8_t* __restrict__ exp_roots,
    const uint32_t* __restrict__ exp_index, const uint8_t* __restrict__ flags, uint8_t* __restrict__ matched,
    const TailSched fin) {
    const uint32_t j = blockIdx.x * kTailBlock + threadIdx.x;
    const uint32_t jj = j < n ? j : n - 1;
    const uint32_t len = lens[jj], pad = pads[jj];
    const bool live = j < n && pad != 0;
    const uint32_t rem = live ? len & 63u : 0u;
    const uint32_t fill = rem ? 64u - rem : 0u;  // zeros that complete the mixed block
    const uint32_t z = live && pad >= fill ? (pad - fill) >> 6 : 0u;
    const uint32_t z_wave = __builtin_amdgcn_readfirstlane(tail_wave_max(z));
    const uint32_t any_pad = __builtin_amdgcn_readfirstlane(tail_wave_max(live ? 1u : 0u));

    State s = iv();
    if (any_pad) {  // wave-uniform
        if (live && (len >> 6)) {
            const uint32_t* st = states + (size_t)jj * 5;
            s = State{st[0], st[1], st[2], st[3], st[4]};
        }
        if (rem) {
            // (as sha1_zero_tail_kernel: only the aligned words that hold a tail byte, the last one masked)
            const uint32_t* q32 = reinterpret_cast<const uint32_t*>(base + tail_offs[jj]);
            uint32_t w[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t off = 4u * k;
                uint32_t v = off < rem ? q32[k] : 0u;
                if (rem - off < 4u) v &= (1u << (8u * (rem - off))) - 1u;
                w[k] = bswap(v);
            }
            compress(s, w);
        }
        for (uint32_t b = 0; b < z_wave; ++b) {
            State t = s;
            compress_known(t, ZeroWords{});
            const bool mine = b < z;
            s.h0 = mine ? t.h0 : s.h0;
            s.h1 = mine ? t.h1 : s.h1;
            s.h2 = mine ? t.h2 : s.h2;
            s.h3 = mine ? t.h3 : s.h3;
            s.h4 = mine ? t.h4 : s.h4;
        }
        compress_known(s, FinalWords{fin});
    }
    if (j >= n) return;
    uint32_t* dg = reinterpret_cast<uint32_t*>(digests + (size_t)j * 20);
    uint32_t d0, d1, d2, d3, d4;
    if (live) {
        d0 = bswap(s.h0), d1 = bswap(s.h1), d2 = bswap(s.h2), d3 = bswap(s.h3), d4 = bswap(s.h4);
        dg[0] = d0;
        dg[1] = d1;
        dg[2] = d2;
        dg[3] = d3;
        dg[4] = d4;
    } else {
        d0 = dg[0], d1 = dg[1], d2 = dg[2], d3 = dg[3], d4 = dg[4];
    }
    const uint32_t fl = flags[j];
    const size_t row = exp_index ? exp_index[j] : j;
    uint32_t verdict = 0;
    if (fl & 1u) {
        const uint32_t* x = reinterpret_cast<const uint32_t*>(exp_sha1 + row * 20);
        verdict |= ((x[0] == d0) & (x[1] == d1) & (x[2] == d2) & (x[3] == d3) & (x[4] == d4)) ? 1u : 0u;
    }
    if (fl & 2u) {
        const uint32_t* r = reinterpret_cast<const uint32_t*>(roots + (size_t)j * 32);
        const uint32_t* x = reinterpret_cast<const uint32_t*>(exp_roots + row * 32);
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) diff |= r[k] ^ x[k];
        verdict |= diff == 0 ? 2u : 0u;
    }
    matched[j] = (uint8_t)verdict;
}

void tail_sched(uint64_t total_len, TailSched* out) {
    uint32_t w[80] = {};
    w[0] = 0x80000000u;
    w[14] = (uint32_t)((total_len * 8u) >> 32);
    w[15] = (uint32_t)(total_len * 8u);
    for (int t = 16; t < 80; ++t) {
        const uint32_t x = w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16];
        w[t] = (x << 1) | (x >> 31);
    }
    for (int t = 0; t < 80; ++t) out->kw[t] = w[t] + (t < 20 ? kK0 : t < 40 ? kK1 : t < 60 ? kK2 : kK3);
}

hipError_t launch_zero_tail(const uint8_t* base, const uint64_t* tail_offs, const uint32_t* lens,
                            const uint32_t* pads, const uint32_t* pids, uint32_t n, uint64_t piece_length,
                            const uint32_t* states, uint8_t* digests, const uint8_t* expected, uint8_t* matched,
                            hipStream_t stream) {
    if (n == 0) return hipSuccess;
    TailSched fin;
    tail_sched(piece_length, &fin);
    const uint32_t blocks = (n + kTailBlock - 1) / kTailBlock;
    hipLaunchKernelGGL(sha1_zero_tail_kernel, dim3(blocks), dim3(kTailBlock), 0, stream, base, tail_offs, lens, pads,
                       pids, n, states, digests, expected, matched, fin);
    return hipGetLastError();
}

hipError_t launch_zero_run(const uint32_t* pids, const uint32_t* poffs, const uint32_t* blocks, uint32_t n,
                           uint32_t* states, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sha1_zero_run_kernel, dim3((n + kTailBlock - 1) / kTailBlock), dim3(kTailBlock), 0, stream, pids,
                       poffs, blocks, n, states);
    return hipGetLastError();
}

hipError_t launch_hybrid_finish(const uint8_t* base, const uint64_t* tail_offs, const uint32_t* lens,
                                const uint32_t* pads, uint32_t n, uint64_t padded_total, const uint32_t* states,
                                uint8_t* digests, const uint8_t* roots, const uint8_t* exp_sha1,
                                const uint8_t* exp_roots, const uint32_t* exp_index, const uint8_t* flags,
                                uint8_t* matched, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    TailSched fin;
    tail_sched(padded_total, &fin);  // (unused when no piece of the launch is padded)
    const uint32_t blocks = (n + kTailBlock - 1) / kTailBlock;
    hipLaunchKernelGGL(hybrid_finish_kernel, dim3(blocks), dim3(kTailBlock), 0, stream, base, tail_offs, lens, pads, n,
                       states, digests, roots, exp_sha1, exp_roots, exp_index, flags, matched, fin);
    return hipGetLastError();
}

hipError_t launch_hybrid_prep(const uint64_t* offsets, const uint32_t* lens, const uint32_t* pads, uint32_t n,
                              uint64_t* tail_offs, uint64_t* poffs, uint64_t* tlens, uint32_t* clens, uint32_t* pids,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_prep_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, offsets, lens,
                       pads, n, tail_offs, poffs, tlens, clens, pids);
    return hipGetLastError();
}

hipError_t launch_hybrid_merge(const uint8_t* v1, const uint8_t* v2, uint32_t n, uint8_t* matched,
                               hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_merge_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, v1, v2, n,
                       matched);
    return hipGetLastError();
}

// SHA-1 of lens[j] zero bytes, from nothing: the digest the
// file re-verify compares an unwritten piece's expected row with, so no byte
// of such a piece is read, staged or copied.  Lane j runs lens[j] >> 6 blocks
// through the tail kernel's zero-block round (to the wave's largest count,
// lanes that are done keep their state under a select), then builds its last
// one or two blocks in registers (lens[j] & 63 zeros, 0x80, the bit length)
// for the general compression: the length need not be a multiple of 64 here,
// so there is no launch-wide final schedule.  Nothing is loaded but lens[j];
// lanes past n redo lane n - 1 (in bounds) and store nothing.
__global__ __launch_bounds__(kTailBlock) void sha1_zero_kernel(const uint32_t* __restrict__ lens, uint32_t n,
                                                               uint8_t* __restrict__ digests) {
    const uint32_t j = blockIdx.x * kTailBlock + threadIdx.x;
    const uint32_t len = lens[j < n ? j : n - 1];
    const uint32_t z = len >> 6, rem = len & 63u;
    const uint32_t z_wave = __builtin_amdgcn_readfirstlane(tail_wave_max(z));

    State s = iv();
    for (uint32_t b = 0; b < z_wave; ++b) {
        State t = s;
        compress_known(t, ZeroWords{});
        const bool mine = b < z;
        s.h0 = mine ? t.h0 : s.h0;
        s.h1 = mine ? t.h1 : s.h1;
        s.h2 = mine ? t.h2 : s.h2;
        s.h3 = mine ? t.h3 : s.h3;
        s.h4 = mine ? t.h4 : s.h4;
    }
    uint32_t w[16];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) w[k] = k == (rem >> 2) ? 0x80000000u >> (8u * (rem & 3u)) : 0u;
    const uint32_t bits_hi = len >> 29, bits_lo = len << 3;
    if (rem <= 55) {  // (0x80 lies in words 0..13: the length's two words are free)
        w[14] = bits_hi;
        w[15] = bits_lo;
    }
    compress(s, w);
    if (rem > 55) {
#pragma unroll
        for (int k = 0; k < 14; ++k) w[k] = 0;
        w[14] = bits_hi;
        w[15] = bits_lo;
        compress(s, w);
    }
    if (j < n) tail_emit(s, j, digests, nullptr, nullptr);
}

hipError_t launch_sha1_zeros(const uint32_t* lens, uint32_t n, uint8_t* digests, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sha1_zero_kernel, dim3((n + kTailBlock - 1) / kTailBlock), dim3(kTailBlock), 0, stream, lens, n,
                       digests);
    return hipGetLastError();
}

}  // namespace vx
