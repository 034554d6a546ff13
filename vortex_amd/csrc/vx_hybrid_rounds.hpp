// vx_hybrid_rounds.hpp — host-only geometry and round planner of the hybrid
// (BEP 52 "upgrade path", v1 + v2) re-verify from disk (vx_hybrid_verify_files
// in vx_hybrid.hip).  No HIP in here: the planner is tested on the CPU
// (tests/native/hybrid_rounds_dump.cpp).
//
// Geometry.  A hybrid torrent pads every file but the last to a piece boundary
// with a BEP 47 pad file, so every file starts its own pieces in v1 as it does
// in v2 and v1 piece i is v2 piece i (vx_merkle::PieceCursor's numbering).  The
// v1 piece that ends a file is its data followed by pad_len = piece_length -
// data_len zeros; the torrent's last piece has no pad.  Pad files are never
// read: the zeros are hashed by the zero-tail kernel without existing anywhere.
//
// Rounds.  The SHA-1 chain of a piece is serial, so the rounds are the chunk
// rounds of the v1 re-verify: a window of consecutive pieces,
// and round k carries chunk k, bytes [kC, (k+1)C), of every piece of the
// window that reaches that far, one SHA-1 lane per piece.  C is a multiple of
// 16 KiB and no piece spans files, so a chunk is also a run of whole merkle
// blocks plus at most its file's tail: chunks sit at 16 KiB stage offsets and
// the same staged bytes feed the merkle block kernel.  A piece shorter than two
// chunks is one chunk.  Per round the planner returns
//  * the reads: one run of one file each (consecutive whole chunks of a file
//    that are also consecutive on the stage merge, up to max_run bytes);
//  * the SHA-1 lanes (launch_chunk's tables): the last data chunk of a padded
//    piece is cut down to whole 64-byte blocks and is not final (its total is
//    piece_length), so the kernel leaves the state; an unpadded piece's last
//    chunk is final.  A lane of 0 bytes is left out;
//  * the tail lanes (launch_zero_tail's tables), for the padded pieces whose
//    data ends in this round;
//  * the block kernel's rows | lens for the stage's blocks, then one entry of
//    length 0 per absent slot of the pieces whose data ends in this round;
//  * whether the round ends its window: then the node kernels reduce the
//    window's n pieces, rows piece-major at the window's widest log2w K (piece
//    p of the window at row p << K).
//
// With a hole predicate the unit is the chunk: chunk k of a
// piece is a hole chunk when its data bytes all lie in ranges the file system
// never wrote.  A hole chunk gets no read and no stage bytes.  For SHA-1,
//  * a piece whose every chunk is a hole has no lane in any round: the caller
//    judges it on the host against SHA-1 of data_len + pad_len zeros (hole_pid
//    / hole_len, given in its window's first round);
//  * a hole chunk in front of a data chunk is a zero-run lane (z_pid, z_poff,
//    z_blocks: launch_zero_run's tables), which takes the piece's state across
//    C bytes of zeros that exist nowhere;
//  * a trailing run of hole chunks [k*, end), k* >= 1, of a piece whose v1
//    total is piece_length is more pad: the piece's tail lane goes out with its
//    last data chunk k* - 1, t_len = k* C and t_pad = piece_length - k* C
//    (nothing of the stage is read: t_len & 63 == 0), and that chunk's lane is
//    not final;
//  * the trailing hole run of the torrent's short, unpadded last piece is read
//    as data: its total is not piece_length, so no tail lane can end it.
// For the merkle side the blocks of a hole chunk are hole_blocks entries in a
// third section of rows | lens, behind the data blocks and the absent slots, as
// in vx_merkle_rounds.hpp: merkle_zero_leaf_kernel writes their rows.  A
// whole-hole piece takes no stage in its window; rows and density count it
// like any piece, so a run of unwritten pieces makes few large windows.
//
// A window closes when round 0 would overflow the stage, when its rows (n + 1)
// << K would pass the row budget, or when it would turn sparse, (n + 1) << K >
// 4 * sum(2^log2w): a torrent of 10^5 tiny files behind one large file does
// not take a full-width tree's rows per tiny file.  Every round's kernels run
// after the previous round's, so one leaf area of row_budget rows and one
// state row per piece serve the whole call.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vx_merkle_rounds.hpp"

namespace vx_hybrid {

using vx_merkle::kBlock;
using vx_merkle::PieceCursor;

constexpr uint64_t kChunk = 256 << 10;      // C of DESIGN.md §6.3
constexpr uint32_t kRowBudget = 1u << 20;   // leaf rows of a window (32 MiB of HBM): DESIGN.md §6.8
constexpr uint64_t kMaxRun = 2ull << 20;    // one pread at most

inline uint64_t align_block(uint64_t x) { return (x + kBlock - 1) / kBlock * kBlock; }

// pad_len of the piece the cursor stands on, in a torrent of n_pieces pieces.
inline uint32_t pad_len(const PieceCursor& pc, uint64_t n_pieces) {
    const uint64_t len = pc.len();
    return len < pc.pl && pc.index + 1 != n_pieces ? (uint32_t)(pc.pl - len) : 0u;
}

// The chunk length of the rounds: C, or the whole piece where a piece is
// shorter than two chunks and fits the stage; a multiple of 16 KiB, 0 when the
// stage holds no block.
inline uint64_t chunk_for(uint32_t piece_length, uint64_t stage_bytes, uint64_t chunk = kChunk) {
    if (piece_length < 2 * chunk && piece_length <= stage_bytes) return piece_length;
    return std::min(chunk, stage_bytes) / kBlock * kBlock;
}

struct Read {
    uint32_t file;
    uint64_t file_off, len, stage_off;
    uint64_t piece;  // the piece of its first byte
};
inline uint64_t stage_offset(const Read& r) { return r.stage_off; }  // (vx_block_rounds.hpp)

struct Round {
    std::vector<Read> reads;
    // SHA-1 lanes: stage offset, offset in the piece, the v1 piece's total length; bytes, piece row
    std::vector<uint64_t> l_off, l_poff, l_tlen;
    std::vector<uint32_t> l_len, l_pid;
    // tail lanes: stage offset of the tail bytes; data_len, pad_len, piece row
    std::vector<uint64_t> t_off;
    std::vector<uint32_t> t_len, t_pad, t_pid;
    // zero-run lanes: piece row, offset in the piece, 64-byte blocks
    std::vector<uint32_t> z_pid, z_poff, z_blocks;
    // the window's whole-hole pieces (in its first round): piece row, v1 total length
    std::vector<uint32_t> hole_pid, hole_len;
    // merkle block entries: data_blocks for the stage's blocks, then the absent slots, then hole_blocks hole blocks
    std::vector<uint32_t> rows, lens;
    uint32_t data_blocks = 0;
    uint32_t hole_blocks = 0;
    uint64_t bytes = 0;  // the stage's extent: what the data copy moves
    uint64_t file_bytes = 0;  // the chunks' bytes, read or not
    uint64_t hole_bytes = 0;  // ... of them, the hole chunks'
    bool new_window = false, end_window = false;
    uint64_t w_first = 0;  // the window: pieces [w_first, w_first + w_n), rows at width w_log2
    uint32_t w_n = 0, w_log2 = 0;
    void clear() { *this = Round{}; }
};

class Rounds {
  public:
    // Pieces [first, first + count) of a torrent of n_pieces pieces; piece rows
    // (l_pid, t_pid, z_pid, hole_pid) count from `first`.  chunk: chunk_for(...),
    // > 0.  hole (may be empty): (file, offset, length) was never written.
    Rounds(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length, uint64_t n_pieces, uint64_t first,
           uint64_t count, uint64_t stage_bytes, uint64_t chunk, uint32_t row_budget = kRowBudget,
           uint64_t max_run = kMaxRun, vx_merkle::HolePredicate hole = nullptr)
        : cur_(file_lengths, nfiles, piece_length), n_pieces_(n_pieces), first_(first), end_(first + count),
          stage_(stage_bytes), C_(chunk), budget_(row_budget), max_run_(max_run), hole_(std::move(hole)) {
        cur_.seek(first);
    }

    bool next(Round& r) {
        r.clear();
        if (k_ == nk_) {
            form_window();
            if (win_.empty()) return false;
            r.new_window = true;
        }
        r.w_first = win_.front().index;
        r.w_n = (uint32_t)win_.size();
        r.w_log2 = K_;
        const uint64_t a = k_ * C_;
        uint64_t at = 0;
        absent_.clear();
        hole_rows_.clear();
        hole_lens_.clear();
        for (size_t p = 0; p < win_.size(); ++p) {
            const Piece& pc = win_[p];
            const uint32_t pid = (uint32_t)(pc.index - first_);
            if (pc.whole && k_ == 0) {
                r.hole_pid.push_back(pid);
                r.hole_len.push_back(pc.data_len + pc.pad_len);
            }
            if (pc.data_len <= a) continue;
            const uint64_t len = std::min<uint64_t>(C_, pc.data_len - a);
            const bool last = a + len == pc.data_len;
            const uint32_t row0 = (uint32_t)(p << K_);
            const uint32_t b0 = (uint32_t)(a / kBlock), nb = (uint32_t)((len + kBlock - 1) / kBlock);
            // a hole chunk: of a whole-hole piece, of a trailing run the tail lane took, or a zero run
            const bool folded = pc.whole || k_ >= pc.k_tail;
            if (folded || (k_ < pc.k_run && hole_(pc.file, pc.file_off + a, (uint32_t)len))) {
                if (!folded) {
                    r.z_pid.push_back(pid);
                    r.z_poff.push_back((uint32_t)a);
                    r.z_blocks.push_back((uint32_t)(len >> 6));  // (a later chunk follows: len == C)
                }
                for (uint32_t j = 0; j < nb; ++j) {
                    hole_rows_.push_back(row0 + b0 + j);
                    hole_lens_.push_back((uint32_t)std::min<uint64_t>(kBlock, len - (uint64_t)j * kBlock));
                }
                if (last)
                    for (uint32_t s = b0 + nb; s < (1u << pc.log2w); ++s) absent_.push_back(row0 + s);
                r.file_bytes += len;
                r.hole_bytes += len;
                continue;
            }
            add_read(r, pc.file, pc.file_off + a, len, at, pc.index);
            const uint64_t slen = pc.pad_len && last ? len & ~63ull : len;
            if (slen) {
                r.l_off.push_back(at);
                r.l_poff.push_back(a);
                r.l_tlen.push_back((uint64_t)pc.data_len + pc.pad_len);
                r.l_len.push_back((uint32_t)slen);
                r.l_pid.push_back(pid);
            }
            if (pc.pad_len && last) {
                r.t_off.push_back(at + slen);
                r.t_len.push_back(pc.data_len);
                r.t_pad.push_back(pc.pad_len);
                r.t_pid.push_back(pid);
            } else if (k_ + 1 == pc.k_tail) {  // the trailing hole run: zeros like the pad's, from here on
                r.t_off.push_back(at);         // (no tail byte: not read)
                r.t_len.push_back((uint32_t)(a + len));
                r.t_pad.push_back((uint32_t)(cur_.pl - (a + len)));
                r.t_pid.push_back(pid);
            }
            for (uint32_t j = 0; j < nb; ++j) {
                r.rows.push_back(row0 + b0 + j);
                r.lens.push_back((uint32_t)std::min<uint64_t>(kBlock, len - (uint64_t)j * kBlock));
            }
            if (last)
                for (uint32_t s = b0 + nb; s < (1u << pc.log2w); ++s) absent_.push_back(row0 + s);
            r.data_blocks += nb;
            r.bytes = at + len;
            r.file_bytes += len;
            at += (uint64_t)nb * kBlock;
        }
        r.rows.insert(r.rows.end(), absent_.begin(), absent_.end());
        r.lens.insert(r.lens.end(), absent_.size(), 0u);
        r.rows.insert(r.rows.end(), hole_rows_.begin(), hole_rows_.end());
        r.lens.insert(r.lens.end(), hole_lens_.begin(), hole_lens_.end());
        r.hole_blocks = (uint32_t)hole_rows_.size();
        if (++k_ == nk_) {
            r.end_window = true;
            win_.clear();
        }
        return true;
    }

  private:
    struct Piece {
        uint64_t index, file_off;
        uint32_t file, data_len, pad_len, log2w;
        // Holes: chunks [0, k_run) ask the predicate; chunks from k_tail on are
        // the trailing hole run its tail lane took (k_tail - 1 carries the lane).
        uint64_t k_run = 0, k_tail = UINT64_MAX;
        bool whole = false;
    };

    // The hole chunks of the piece the cursor stands on.
    void classify(Piece& pc) const {
        if (!hole_ || pc.data_len == 0) return;
        const uint64_t nck = (pc.data_len + C_ - 1) / C_;
        uint64_t t = nck;  // the trailing hole run is chunks [t, nck)
        while (t && hole_(pc.file, pc.file_off + (t - 1) * C_,
                          (uint32_t)std::min<uint64_t>(C_, pc.data_len - (t - 1) * C_)))
            --t;
        pc.whole = t == 0;
        pc.k_run = t;
        // (a short unpadded last piece's total is not piece_length: its run is read)
        if (t && t < nck && (uint64_t)pc.data_len + pc.pad_len == cur_.pl) pc.k_tail = t;
    }

    void form_window() {
        win_.clear();
        k_ = nk_ = 0;
        K_ = 0;
        uint64_t used = 0, S = 0, longest = 0;
        while (!cur_.end() && cur_.index < end_) {
            const uint32_t len = (uint32_t)cur_.len(), lw = cur_.log2w();
            Piece pc{cur_.index, cur_.off(), (uint32_t)cur_.f, len, pad_len(cur_, n_pieces_), lw};
            classify(pc);
            const uint64_t need = pc.whole ? 0 : align_block(std::min<uint64_t>(C_, len));
            const uint32_t K2 = std::max(K_, lw);
            const uint64_t n = win_.size(), rows = (n + 1) << K2;
            if (n && (used + need > stage_ || rows > budget_ || rows > 4 * (S + (1ull << lw)))) break;
            win_.push_back(pc);
            used += need;
            S += 1ull << lw;
            K_ = K2;
            longest = std::max<uint64_t>(longest, len);
            cur_.next();
        }
        nk_ = win_.empty() ? 0 : (longest + C_ - 1) / C_;
    }

    void add_read(Round& r, uint32_t file, uint64_t off, uint64_t len, uint64_t at, uint64_t piece) const {
        if (!r.reads.empty()) {
            Read& p = r.reads.back();
            if (p.file == file && p.file_off + p.len == off && p.stage_off + p.len == at && p.len + len <= max_run_) {
                p.len += len;
                return;
            }
        }
        r.reads.push_back(Read{file, off, len, at, piece});
    }

    PieceCursor cur_;
    const uint64_t n_pieces_, first_, end_, stage_, C_;
    const uint32_t budget_;
    const uint64_t max_run_;
    std::vector<Piece> win_;
    uint64_t k_ = 0, nk_ = 0;  // the next round of the window, its rounds
    uint32_t K_ = 0;
    std::vector<uint32_t> absent_;
    const vx_merkle::HolePredicate hole_;
    std::vector<uint32_t> hole_rows_, hole_lens_;
};

}  // namespace vx_hybrid
