// vx_merkle_leaves.hpp — host-only layout of a v2 torrent's leaf table (the
// 16 KiB leaf layer that vx_merkle_verify_files_blocks checks against and
// vx_merkle_hash_files_leaves hands out, DESIGN.md §3.7 "Block checks from
// disk").  No HIP in here: the layout is tested on the CPU
// (tests/native/leaf_layout_dump.cpp).
//
// The table is the files' leaf layers back to back, in file order: file f
// contributes ceil(len_f / 16 KiB) rows of 32 bytes, an empty file none, and
// there is no padding row anywhere.  With leaf_off[f] the rows of the files in
// front of f, the first row of piece i (piece j of file f) is
//   leaf_first(i) = leaf_off[f] + j * (piece_length / 16 KiB)
// and the piece has ceil(piece_len(i) / 16 KiB) rows, so the rows of a range of
// pieces are one run of the table.
#pragma once
#include <stdint.h>

#include <vector>

#include "vx_merkle_rounds.hpp"

namespace vx_merkle {

inline uint64_t file_leaves(uint64_t len) { return (len + kBlock - 1) / kBlock; }

// Rows of the whole torrent's leaf table.
inline uint64_t torrent_leaf_rows(const uint64_t* lens, size_t nfiles) {
    uint64_t n = 0;
    for (size_t f = 0; f < nfiles; ++f) n += file_leaves(lens[f]);
    return n;
}

// The leaf rows of pieces [first, first + count): rows [base, base + rows) of
// the table; piece k of the range has blocks[k] rows from row base +
// leaf_first[k] on.
struct LeafRange {
    uint64_t base = 0, rows = 0;
    std::vector<uint32_t> leaf_first, blocks;
};

// false: the range's rows number 2^32 or more (out is then unspecified).
inline bool leaf_range(const uint64_t* lens, size_t nfiles, uint32_t piece_length, uint64_t first, uint64_t count,
                       LeafRange& out) {
    out = LeafRange{};
    PieceCursor pc(lens, nfiles, piece_length);
    pc.seek(first);
    if (count == 0 || pc.end()) return true;
    uint64_t leaf_off = 0;  // of the cursor's file
    for (size_t f = 0; f < pc.f; ++f) leaf_off += file_leaves(lens[f]);
    const uint64_t width = piece_length / kBlock;
    out.base = leaf_off + pc.j * width;
    out.leaf_first.reserve(count);
    out.blocks.reserve(count);
    size_t file = pc.f;
    for (uint64_t i = 0; i < count && !pc.end(); ++i, pc.next()) {
        for (; file < pc.f; ++file) leaf_off += file_leaves(lens[file]);
        const uint64_t at = leaf_off + pc.j * width - out.base;
        if ((at + pc.blocks()) >> 32) return false;
        out.leaf_first.push_back((uint32_t)at);
        out.blocks.push_back(pc.blocks());
        out.rows = at + pc.blocks();
    }
    return true;
}

}  // namespace vx_merkle
