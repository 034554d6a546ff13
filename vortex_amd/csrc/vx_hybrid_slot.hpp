// vx_hybrid_slot.hpp — the host-only part of the hybrid download path
// (vx_hybrid_submit): the argument check of one piece, the
// values its lane takes in the chunked SHA-1 kernel and the finish kernel, and
// where a launch's metadata lies in the slot's one packed block (vx_slots.hip
// submits and launches with them).  No HIP
// dependency: tests/native/hybrid_slot_dump.cpp runs it as a stand-alone
// program under ASan + UBSan against a Python model.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "vx_hash.h"

namespace vx_hybrid_slot {

// max_piece_len rounded up to a power of two, VX_MERKLE_BLOCK at least: the
// widest tree and the largest padded total a context takes.
inline uint64_t widest_piece(uint32_t max_piece_len) {
    uint64_t w = VX_MERKLE_BLOCK;
    while (w < max_piece_len) w <<= 1;
    return w;
}

// The check of vx_hybrid_submit's numbers (vx_hash.h), and with pad_len = 0
// of vx_merkle_submit's: 0, or VX_ERANGE / VX_EINVAL with *why set.
inline int check(uint32_t len, uint32_t pad_len, uint32_t log2w, uint32_t max_piece_len, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (len > max_piece_len) return *why = "piece longer than max_piece_len", VX_ERANGE;
    if (log2w > VX_MERKLE_MAX_LOG2_WIDTH) return *why = "log2w > 17", VX_EINVAL;
    const uint64_t tree = (uint64_t)VX_MERKLE_BLOCK << log2w, widest = widest_piece(max_piece_len);
    if (len > tree) return *why = "piece longer than its tree (16384 << log2w)", VX_EINVAL;
    if (tree > widest) return *why = "tree wider than max_piece_len", VX_EINVAL;
    if (pad_len == 0) return 0;
    if (len == 0) return *why = "a pad behind an empty piece", VX_EINVAL;
    const uint64_t total = (uint64_t)len + pad_len;
    if (total & (total - 1)) return *why = "len + pad_len is not a power of two", VX_EINVAL;
    if (total < VX_MERKLE_BLOCK || total < tree) return *why = "len + pad_len is below the piece's tree", VX_EINVAL;
    if (total > widest) return *why = "len + pad_len is above max_piece_len", VX_EINVAL;
    return 0;
}

// One piece's lane: `off` is where its data starts in the slot's arena.
struct Lane {
    uint64_t tail_off;  // arena offset of the bytes behind the whole 64-byte blocks (4-byte aligned when off is)
    uint64_t total;     // the v1 message length: len + pad
    uint32_t chunk;     // bytes the chunked kernel hashes: a padded piece's whole blocks, else the piece
    uint32_t pad;
    uint32_t zero_blocks;  // all-zero 64-byte blocks between the mixed block and the final padding block
    uint8_t mixed;         // 1: len & 63 tail bytes and zeros share one block
    uint8_t flags;         // bit 0: compare the SHA-1, bit 1: compare the root
};

inline Lane lane(uint64_t off, uint32_t len, uint32_t pad, uint8_t flags) {
    Lane l{};
    l.tail_off = off + (len & ~63u);
    l.total = (uint64_t)len + pad;
    l.chunk = pad ? len & ~63u : len;
    l.pad = pad;
    const uint32_t rem = pad ? len & 63u : 0u;
    const uint32_t fill = rem ? 64u - rem : 0u;  // zeros that complete the mixed block (pad >= fill: total % 64 == 0)
    l.zero_blocks = pad ? (pad - fill) >> 6 : 0u;
    l.mixed = rem != 0;
    l.flags = flags;
    return l;
}

// A launch's metadata for n pieces is one block, copied to the device in one
// H2D: uint64 columns, then uint32 ones, then byte rows; the SHA-1 states
// follow on the device only.  Every offset is a multiple of 16.
struct Pack {
    size_t offsets, tail_offs, totals, poffs, src;    // uint64 x n (poffs: zeros, every chunk starts its piece)
    size_t lens, pads, chunks, ident, rows, tfirst;   // uint32 x n (ident: 0..n-1; tfirst: n + 1)
    size_t exp_sha1, exp_roots, flags, log2w;         // 20n, 32n, n, n bytes
    size_t copy_bytes;                                // the H2D ends here
    size_t states;                                    // 20n bytes, device only
    size_t bytes;
};

inline Pack pack(uint32_t n) {
    Pack p{};
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t was = at;
        at = (at + bytes + 15) / 16 * 16;
        return was;
    };
    const size_t m = n;
    p.offsets = take(m * 8);
    p.tail_offs = take(m * 8);
    p.totals = take(m * 8);
    p.poffs = take(m * 8);
    p.src = take(m * 8);
    p.lens = take(m * 4);
    p.pads = take(m * 4);
    p.chunks = take(m * 4);
    p.ident = take(m * 4);
    p.rows = take(m * 4);
    p.tfirst = take(m * 4 + 4);
    p.exp_sha1 = take(m * 20);
    p.exp_roots = take(m * 32);
    p.flags = take(m);
    p.log2w = take(m);
    p.copy_bytes = at;
    p.states = take(m * 20);
    p.bytes = at;
    return p;
}

}  // namespace vx_hybrid_slot
