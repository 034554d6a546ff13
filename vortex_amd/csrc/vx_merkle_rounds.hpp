// vx_merkle_rounds.hpp — host-only round packer of the BitTorrent v2 re-verify
// from disk (vx_merkle_verify_files in vx_merkle_files.hip).  No HIP in here: the
// packer is tested on the CPU (tests/native/merkle_rounds_dump.cpp).
//
// A v2 piece's 16 KiB blocks are independent, so a round is any run of blocks:
// the packer walks the pieces of a range in order and fills one round after
// another with their blocks, cutting a round wherever its stage is full
// (mid-piece, mid-file).  Per round it returns
//  * the reads: runs of consecutive blocks of one file, each starting at a
//    block boundary of its file and at stage block `stage_block` (16 KiB
//    aligned, so an O_DIRECT read can take it); a file's short last block is
//    followed by the next file at the next stage block;
//  * the block kernel's tables: rows[b] / lens[b] for stage block b, then, past
//    the data blocks, one entry of length 0 per absent slot (a slot of a
//    piece's tree beyond its last block) of the pieces the round finished;
//  * the node launches: the groups of pieces the round finished.
// With a hole predicate a block the file system never wrote
// gets no read and no stage block: it becomes an entry (row, length) in a third
// section of the tables, behind the data blocks and the absent slots, whose
// leaf row is SHA-256(length zero bytes) by a kernel of its own.  Window and
// group rules count its row like any row.
//
// Leaf rows live in a ring of `window_rows` rows (a power of two).  The node
// kernels reduce pieces laid out piece-major at one width per launch, so the
// pieces are cut into groups: consecutive pieces, rows of piece k of a group at
// base + (k << K), K = the widest log2w of the group.  A piece joins a group
// while the group stays dense, (n+1) << K <= 4 * sum(2^log2w), and small,
// (n+1) << K <= window_rows / 4; the first keeps a torrent of many small files
// from taking a full-width tree's rows per file, the second keeps a group in
// the window.  A group's base is aligned to 2^K in an unbounded row count whose
// low bits are the ring position, so no piece wraps; a group that wraps is two
// launches.  Groups finish in order (blocks go in order), so one group is open
// at a time.  A round is also cut before a group that would put more than
// window_rows between the oldest unfinished group's base and its own end: the
// kernels of round k run after those of round k-1, so every row a later node
// launch reads lies in that span and no two rows of it share a ring position.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace vx_merkle {

constexpr uint32_t kBlock = 16384;  // VX_MERKLE_BLOCK
constexpr uint32_t kSkipRow = 0xFFFFFFFFu;
constexpr uint32_t kMaxLog2Width = 17;  // VX_MERKLE_MAX_LOG2_WIDTH

inline uint32_t log2_ceil(uint64_t x) {
    uint32_t k = 0;
    while ((1ull << k) < x) ++k;
    return k;
}

inline uint64_t file_pieces(uint64_t len, uint32_t piece_length) {
    return (len + piece_length - 1) / piece_length;
}

inline uint64_t torrent_pieces(const uint64_t* lens, size_t nfiles, uint32_t piece_length) {
    uint64_t n = 0;
    for (size_t f = 0; f < nfiles; ++f) n += file_pieces(lens[f], piece_length);
    return n;
}

// The pieces of a torrent in order: piece j of file f is torrent piece `index`.
struct PieceCursor {
    const uint64_t* lens = nullptr;
    size_t nfiles = 0;
    uint32_t pl = kBlock;
    size_t f = 0;
    uint64_t j = 0, index = 0;

    PieceCursor(const uint64_t* file_lengths, size_t n, uint32_t piece_length)
        : lens(file_lengths), nfiles(n), pl(piece_length) {
        settle();
    }
    bool end() const { return f >= nfiles; }
    uint64_t off() const { return j * pl; }
    uint64_t len() const { return std::min<uint64_t>(pl, lens[f] - j * pl); }
    uint32_t blocks() const { return (uint32_t)((len() + kBlock - 1) / kBlock); }
    uint32_t log2w() const { return lens[f] > pl ? log2_ceil(pl / kBlock) : log2_ceil(blocks()); }
    void next() {
        ++j;
        ++index;
        settle();
    }
    void seek(uint64_t piece) {
        f = 0;
        j = index = 0;
        while (f < nfiles) {
            const uint64_t n = file_pieces(lens[f], pl);
            if (piece < index + n) {
                j = piece - index;
                index = piece;
                return;
            }
            index += n;
            ++f;
        }
    }

  private:
    void settle() {
        while (f < nfiles && j >= file_pieces(lens[f], pl)) {
            ++f;
            j = 0;
        }
    }
};

// One pread: len bytes of file `file` from file_off, to stage block
// stage_block on; `piece` is the torrent piece of its first block (the later
// blocks' pieces follow from file_off and the piece length).
struct Read {
    uint32_t file;
    uint64_t file_off, len;
    uint32_t stage_block;
    uint64_t piece;
};
inline uint64_t stage_offset(const Read& r) { return (uint64_t)r.stage_block * kBlock; }  // in bytes (vx_block_rounds.hpp)

// One node launch: pieces [first, first + n), piece k's rows at ring row
// row0 + (k << log2_width).
struct Nodes {
    uint64_t first;
    uint32_t n, log2_width, row0;
};

struct Round {
    std::vector<Read> reads;
    // data_blocks entries for the stage's blocks, then the absent slots, then hole_blocks entries for the hole blocks
    std::vector<uint32_t> rows, lens;
    uint32_t data_blocks = 0;
    uint32_t hole_blocks = 0;
    uint64_t bytes = 0;  // the stage's extent: what the data copy moves
    uint64_t file_bytes = 0;  // the blocks' bytes, read or not
    uint64_t hole_bytes = 0;  // ... of them, the hole blocks'
    std::vector<Nodes> nodes;
    void clear() {
        reads.clear();
        rows.clear();
        lens.clear();
        nodes.clear();
        data_blocks = hole_blocks = 0;
        bytes = file_bytes = hole_bytes = 0;
    }
};

// (file, offset in it, length): the whole block was never written.
using HolePredicate = std::function<bool(uint32_t, uint64_t, uint32_t)>;

class Rounds {
  public:
    // Pieces [first, first + count) of the torrent; a round holds at most
    // blocks_per_round stage blocks and max_entries table entries (at least
    // blocks_per_round + piece_length / 16 KiB, so an empty round takes any
    // piece's end); a read is at most max_run_blocks long.  hole (may be empty):
    // the blocks to leave unread.
    Rounds(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length, uint64_t first, uint64_t count,
           uint32_t blocks_per_round, uint32_t window_rows, uint32_t max_entries, uint32_t max_run_blocks,
           HolePredicate hole = nullptr)
        : cur_(file_lengths, nfiles, piece_length), end_(first + count), bpr_(blocks_per_round), R_(window_rows),
          max_entries_(max_entries), max_run_(std::max<uint32_t>(1, max_run_blocks)), hole_(std::move(hole)) {
        cur_.seek(first);
    }

    // The smallest window the packer takes for these rounds: every group fits
    // a quarter of it.
    static uint32_t window_for(uint32_t blocks_per_round, uint32_t piece_length) {
        const uint64_t w = piece_length / kBlock;
        return 1u << log2_ceil(16 * std::max<uint64_t>(blocks_per_round, w));
    }

    // Fill r with the next round; false when the range is done.
    bool next(Round& r) {
        r.clear();
        absent_.clear();
        hole_rows_.clear();
        hole_lens_.clear();
        if (cur_.end() || cur_.index >= end_) return false;
        uint64_t live_lo = open_ ? g_base_ : 0;
        bool have_lo = open_;
        while (!cur_.end() && cur_.index < end_ && r.data_blocks < bpr_) {
            if (!open_) {
                uint64_t n = 0, K = 0;
                form_group(n, K);
                const uint64_t base = (alloc_ + (1ull << K) - 1) >> K << K;
                if (have_lo && base + (n << K) - live_lo > R_) break;  // the window: cut here
                if (!have_lo) {
                    live_lo = base;
                    have_lo = true;
                }
                g_first_ = cur_.index;
                g_n_ = n;
                g_K_ = (uint32_t)K;
                g_base_ = base;
                g_done_ = 0;
                alloc_ = base + (n << K);
                open_ = true;
            }
            const uint32_t nb = cur_.blocks();
            const uint64_t plen = cur_.len();
            // the blocks that fit: to the piece's end, or to the first data block the stage has no room for
            uint32_t take = std::min<uint32_t>(nb - blk_, bpr_ - r.data_blocks);
            if (hole_) {
                uint32_t room = bpr_ - r.data_blocks;
                for (take = 0; blk_ + take < nb; ++take) {
                    const uint64_t at = (uint64_t)(blk_ + take) * kBlock;
                    if (is_hole(at, plen)) continue;
                    if (room == 0) break;
                    --room;
                }
            }
            const bool completes = blk_ + take == nb;
            const uint64_t absent = completes ? (1ull << cur_.log2w()) - nb : 0;
            const uint64_t entries = r.rows.size() + absent_.size() + hole_rows_.size();
            if (entries && entries + take + absent > max_entries_) break;  // the tables: cut here
            const uint64_t piece_row = g_base_ + ((cur_.index - g_first_) << g_K_);
            for (uint32_t k = 0; k < take; ++k) {
                const uint64_t at = (uint64_t)(blk_ + k) * kBlock;
                const uint32_t len = (uint32_t)std::min<uint64_t>(kBlock, plen - at);
                if (hole_ && is_hole(at, plen)) {
                    hole_rows_.push_back(ring(piece_row + blk_ + k));
                    hole_lens_.push_back(len);
                    r.file_bytes += len;
                    r.hole_bytes += len;
                    continue;
                }
                add_read(r, (uint32_t)cur_.f, cur_.off() + at, len, cur_.index);
                r.rows.push_back(ring(piece_row + blk_ + k));
                r.lens.push_back(len);
                r.bytes = (uint64_t)r.data_blocks * kBlock + len;
                r.file_bytes += len;
                ++r.data_blocks;
            }
            blk_ += take;
            if (!completes) continue;  // (the stage is full)
            for (uint64_t s = nb; s < nb + absent; ++s) absent_.push_back(ring(piece_row + s));
            blk_ = 0;
            cur_.next();
            if (++g_done_ == g_n_) {
                emit_group(r);
                open_ = false;
            }
        }
        r.rows.insert(r.rows.end(), absent_.begin(), absent_.end());
        r.lens.insert(r.lens.end(), absent_.size(), 0u);
        r.rows.insert(r.rows.end(), hole_rows_.begin(), hole_rows_.end());
        r.lens.insert(r.lens.end(), hole_lens_.begin(), hole_lens_.end());
        r.hole_blocks = (uint32_t)hole_rows_.size();
        return true;
    }

  private:
    uint32_t ring(uint64_t row) const { return (uint32_t)(row & (R_ - 1)); }

    // the block at byte `at` of the current piece (plen bytes)
    bool is_hole(uint64_t at, uint64_t plen) const {
        return hole_((uint32_t)cur_.f, cur_.off() + at, (uint32_t)std::min<uint64_t>(kBlock, plen - at));
    }

    void form_group(uint64_t& n, uint64_t& K) const {
        PieceCursor lk = cur_;
        uint64_t S = 0;
        n = K = 0;
        while (!lk.end() && lk.index < end_) {
            const uint64_t lw = lk.log2w(), K2 = std::max(K, lw);
            if (n && (((n + 1) << K2) > 4 * (S + (1ull << lw)) || ((n + 1) << K2) > R_ / 4)) break;
            ++n;
            K = K2;
            S += 1ull << lw;
            lk.next();
        }
    }

    void add_read(Round& r, uint32_t file, uint64_t off, uint32_t len, uint64_t piece) const {
        if (!r.reads.empty()) {
            Read& p = r.reads.back();
            if (p.file == file && p.file_off + p.len == off && p.len % kBlock == 0 &&
                p.stage_block + p.len / kBlock == r.data_blocks && p.len / kBlock < max_run_) {
                p.len += len;
                return;
            }
        }
        r.reads.push_back(Read{file, off, len, r.data_blocks, piece});
    }

    void emit_group(Round& r) const {
        const uint64_t start = g_base_ & (R_ - 1), rows = g_n_ << g_K_;
        if (start + rows <= R_) {
            r.nodes.push_back(Nodes{g_first_, (uint32_t)g_n_, g_K_, (uint32_t)start});
            return;
        }
        const uint64_t n1 = (R_ - start) >> g_K_;  // base is 2^K aligned: the wrap falls between two pieces
        r.nodes.push_back(Nodes{g_first_, (uint32_t)n1, g_K_, (uint32_t)start});
        r.nodes.push_back(Nodes{g_first_ + n1, (uint32_t)(g_n_ - n1), g_K_, 0});
    }

    PieceCursor cur_;
    const uint64_t end_;
    const uint32_t bpr_;
    const uint64_t R_;
    const uint64_t max_entries_;
    const uint32_t max_run_;
    uint32_t blk_ = 0;  // blocks of the current piece already placed
    bool open_ = false;
    uint64_t g_first_ = 0, g_n_ = 0, g_base_ = 0, g_done_ = 0, alloc_ = 0;
    uint32_t g_K_ = 0;
    std::vector<uint32_t> absent_;
    const HolePredicate hole_;
    std::vector<uint32_t> hole_rows_, hole_lens_;
};

}  // namespace vx_merkle
