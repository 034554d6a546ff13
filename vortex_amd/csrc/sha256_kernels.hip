// sha256_kernels.hip — BitTorrent v2 (BEP 52) piece verification for MI355X
// (gfx950): SHA-256 merkle trees over 16 KiB blocks.
//
// Mapping:
//  * leaf kernel: one lane per leaf slot.  Lane g serves piece g >> log2_width,
//    slot g & (width-1); a 16 MiB piece is 1,024 independent lanes where the
//    SHA-1 kernels have one chain.  A lane streams its block in 128-byte
//    groups (one L2 line, two SHA-256 blocks) with 8 x global_load_dwordx4,
//    one group ahead of the compression in a register ring (two groups of
//    compression, ~2,800 VALU, cover an HBM miss many times over); the loop
//    bound is wave-uniform, the ring indices compile-time (no scratch).  The
//    tail of a short leaf is read byte-exactly: no load touches a byte past
//    the piece's end.  A slot that starts at or past the piece's end gets the
//    zero hash and hashes nothing.  The padding block of a full leaf is a
//    compile-time constant (rounds only).
//  * node kernel: 256 threads reduce a tile of 512 rows in LDS, one node
//    (two compressions, the second a constant padding block) per thread and
//    level.  Trees up to 512 leaves share a tile (512 >> log2_width pieces per
//    workgroup); wider ones take one workgroup per piece, which reduces the
//    piece tile by tile and then the tiles' tops.  Under 1 % of the leaf work.
//  * layer kernel (vx_merkle_device_root): the same tile reduction over a
//    layer of n hashes, missing rows filled with the pad hash of the level.
//  * layers kernel (vx_merkle_device_layers): that reduction over many layers
//    at once, one workgroup per tile of a plan the host made
//    (vx_merkle_layers.hpp), one launch per pass.
//  * proof kernels (vx_merkle_device_proofs): a workgroup per proof reduces its
//    span in the same tile, then a lane per proof walks the uncles.
//  * piece kernel (vx_merkle_device_pieces, the async path of
//    vx_merkle_submit): the leaf kernel's lanes with the tree fused on.  A
//    workgroup's 256 leaf rows stay in LDS and are reduced there; trees of at
//    most 256 leaves finish in the one launch, wider ones leave a top per
//    256-leaf tile for the node kernel.  No leaf layer is kept.
//  * zero-copy piece kernel (vx_set_merkle_zero_copy): the piece kernel with
//    each piece at a device-visible address of its own (a registered host
//    buffer's mapping) and a cooperative leaf phase: a wave loads 256 bytes of
//    each of its 64 leaves per tile, two tiles in flight, and transposes them
//    through LDS to the lane that owns the leaf.  The tree phase is shared.
//  * block check kernel (vx_merkle_device_block_check): the leaf kernel's
//    lanes, each comparing its leaf with an expected row; a wave's verdicts
//    leave as one ballot, a bit per 16 KiB block.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sha256_device.hpp"
#include "vx_kernels.h"

namespace vx {
namespace {

using sha256::State;

constexpr uint32_t kLeaf = 16384;       // VX_MERKLE_BLOCK
constexpr int kTileLog2 = 9;            // rows a workgroup reduces at once: 512 x 32 B = 16 KiB of LDS
constexpr uint32_t kTile = 1u << kTileLog2;
constexpr int kNodeBlock = kTile / 2;   // one thread per node of the tile's first level
constexpr int kMaxTops = 1 << (kMerkleMaxLog2Width - kTileLog2);

__device__ constexpr sha256::ConstBlock kPadLeaf = sha256::pad_block(kLeaf);  // after a full 16 KiB leaf
__device__ constexpr sha256::ConstBlock kPadNode = sha256::pad_block(64);     // after left || right

// A line of zeros: the load target for lanes that have no full group to
// stream, so every issued load stays in bounds.
__device__ __attribute__((aligned(128))) uint4 g_zero_group[8];

__device__ __forceinline__ void load_group(uint4 (&dst)[8], const uint4* src) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = src[k];
}

__device__ __forceinline__ void compress_group(State& s, const uint4 (&g)[8]) {
    sha256::compress_le(s, g[0], g[1], g[2], g[3]);
    sha256::compress_le(s, g[4], g[5], g[6], g[7]);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// Stream `ng` 128-byte groups from src with a 2-deep register ring.  ng_wave:
// the wave-wide loop bound; lanes with ng < ng_wave keep issuing (clamped,
// in-bounds) loads and skip the compression.
__device__ __forceinline__ void stream_groups(State& s, const uint4* src, uint32_t ng, uint32_t ng_wave) {
    if (ng_wave == 0) return;
    const uint4* base = ng ? src : g_zero_group;
    const uint32_t last = ng ? ng - 1 : 0;
    uint4 ring[2][8];
    load_group(ring[0], base);
    for (uint32_t g0 = 0; g0 < ng_wave; g0 += 2) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t gl_raw = g0 + r + 1;
            const uint32_t gl = gl_raw < last ? gl_raw : last;
            load_group(ring[r ^ 1], base + (size_t)gl * 8);
            if (g0 + r < ng) compress_group(s, ring[r]);
        }
    }
}

// The last rem (< 128) bytes at q (16-byte aligned) of a message of total
// bytes, then the FIPS 180-4 padding: 1 to 3 blocks, built word by word from
// bytes inside [q, q+rem) only.  One compression in a loop: this runs once
// per short leaf, and unrolled it would triple the kernel's code.
__device__ __forceinline__ void finish_tail(State& s, const uint8_t* q, uint32_t rem, uint32_t total) {
    const uint32_t* q32 = reinterpret_cast<const uint32_t*>(q);
    const uint32_t nblk = (rem + 9 + 63) >> 6;
#pragma nounroll
    for (uint32_t b = 0; b < nblk; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t off = 64u * b + 4u * k;
            uint32_t v = 0;
            if (off + 4 <= rem) {
                v = q32[off >> 2];
            } else if (off < rem) {
                for (uint32_t j = 0; off + j < rem; ++j) v |= (uint32_t)q[off + j] << (8 * j);
            }
            if (rem >= off && rem < off + 4) v |= 0x80u << (8 * (rem - off));
            w[k] = sha256::bswap(v);
        }
        if (b + 1 == nblk) w[15] = total * 8u;  // a leaf is at most 16 KiB: the high word stays 0
        sha256::compress(s, w);
    }
}

__device__ __forceinline__ void store_row(uint8_t* rows, uint32_t row, const State& s) {
    uint4* o = reinterpret_cast<uint4*>(rows + (size_t)row * 32);
    o[0] = make_uint4(sha256::bswap(s.h[0]), sha256::bswap(s.h[1]), sha256::bswap(s.h[2]), sha256::bswap(s.h[3]));
    o[1] = make_uint4(sha256::bswap(s.h[4]), sha256::bswap(s.h[5]), sha256::bswap(s.h[6]), sha256::bswap(s.h[7]));
}

// Lane g: leaf slot g & (width-1) of piece g >> log2_width.  kRagged: piece i
// at base + offsets[i], lens[i] bytes; else at base + i*stride, len bytes, the
// last piece last_len.
template <bool kRagged>
__global__ __launch_bounds__(kBlock) void merkle_leaf_kernel(const uint8_t* __restrict__ base, uint64_t stride,
                                                             uint32_t len, uint32_t last_len,
                                                             const uint64_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ lens, uint32_t n,
                                                             uint32_t log2_width, uint8_t* __restrict__ leaves) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t rows = n << log2_width;
    // Lanes past the last row redo row rows-1 (in bounds, the wave stays
    // convergent) and store nothing.
    const uint32_t gg = g < rows ? g : rows - 1;
    const uint32_t piece = gg >> log2_width;
    const uint32_t slot = gg & ((1u << log2_width) - 1);
    const uint32_t plen = kRagged ? lens[piece] : (piece == n - 1 ? last_len : len);
    const uint8_t* p = base + (kRagged ? offsets[piece] : (uint64_t)piece * stride);
    const uint64_t start = (uint64_t)slot * kLeaf;
    const uint32_t leaf_len = start < plen ? (plen - start < kLeaf ? (uint32_t)(plen - start) : kLeaf) : 0;
    const uint32_t ng = leaf_len >> 7;
    const uint32_t ng_wave = __builtin_amdgcn_readfirstlane(wave_max(ng));
    p += start < plen ? start : 0;
    State s = sha256::iv();
    stream_groups(s, reinterpret_cast<const uint4*>(p), ng, ng_wave);
    if (leaf_len == kLeaf) {
        sha256::compress_const(s, kPadLeaf);
    } else if (leaf_len) {
        finish_tail(s, p + (size_t)ng * 128, leaf_len & 127u, leaf_len);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) s.h[k] = 0;  // beyond the piece: the zero hash, not a hash of anything
    }
    if (g < rows) store_row(leaves, g, s);
}

// Block check (vx_merkle_device_block_check, DESIGN.md §3.7 "Block checks"):
// the lanes and the streaming of merkle_leaf_kernel<true>, but each lane
// compares its digest with row g of expected_leaves and a wave's verdicts
// leave as one ballot.  Bitmap: uint64 words, max(1, W/64) per piece, block b
// of piece i = bit b & 63 of word i * wpp + (b >> 6).
//  * W >= 64: a wave is 64 consecutive slots of one piece, its ballot is one
//    whole word; lane 0 stores it.
//  * W < 64: a wave holds 64 / W whole pieces; the lane of each piece's slot 0
//    shifts the ballot down to its own bit and stores the piece's W bits.
// Every word has exactly one writing lane (no atomics, no LDS) and every word
// of pieces [0, n) is written, zeros included.  A slot at or past the piece's
// end is never bad.  The expected row is loaded after the hashing: it is not
// live across the streaming loop.  expected_leaves NULL: leaves_out only.
__global__ __launch_bounds__(kBlock) void merkle_block_check_kernel(const uint8_t* __restrict__ base,
                                                                    const uint64_t* __restrict__ offsets,
                                                                    const uint32_t* __restrict__ lens, uint32_t n,
                                                                    uint32_t log2_width,
                                                                    const uint8_t* __restrict__ expected_leaves,
                                                                    unsigned long long* __restrict__ bad_words,
                                                                    uint8_t* __restrict__ leaves_out) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t rows = n << log2_width;
    // Lanes past the last row redo row rows-1 (in bounds, the wave stays
    // convergent), store nothing and contribute 0 to the ballot.
    const uint32_t gg = g < rows ? g : rows - 1;
    const uint32_t piece = gg >> log2_width;
    const uint32_t slot = gg & ((1u << log2_width) - 1);
    const uint32_t plen = lens[piece];
    const uint8_t* p = base + offsets[piece];
    const uint64_t start = (uint64_t)slot * kLeaf;
    const uint32_t leaf_len = start < plen ? (plen - start < kLeaf ? (uint32_t)(plen - start) : kLeaf) : 0;
    const uint32_t ng = leaf_len >> 7;
    const uint32_t ng_wave = __builtin_amdgcn_readfirstlane(wave_max(ng));
    p += start < plen ? start : 0;
    State s = sha256::iv();
    stream_groups(s, reinterpret_cast<const uint4*>(p), ng, ng_wave);
    if (leaf_len == kLeaf) {
        sha256::compress_const(s, kPadLeaf);
    } else if (leaf_len) {
        finish_tail(s, p + (size_t)ng * 128, leaf_len & 127u, leaf_len);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) s.h[k] = 0;  // beyond the piece: the zero hash, not a hash of anything
    }
    if (leaves_out && g < rows) store_row(leaves_out, g, s);
    if (!expected_leaves) return;  // (kernel-uniform)
    asm volatile("" ::: "memory");  // the row's loads stay below the hashing
    const uint4* x = reinterpret_cast<const uint4*>(expected_leaves + (size_t)gg * 32);
    const uint4 x0 = x[0], x1 = x[1];
    const uint32_t diff = (x0.x ^ sha256::bswap(s.h[0])) | (x0.y ^ sha256::bswap(s.h[1])) |
                          (x0.z ^ sha256::bswap(s.h[2])) | (x0.w ^ sha256::bswap(s.h[3])) |
                          (x1.x ^ sha256::bswap(s.h[4])) | (x1.y ^ sha256::bswap(s.h[5])) |
                          (x1.z ^ sha256::bswap(s.h[6])) | (x1.w ^ sha256::bswap(s.h[7]));
    const bool bad = g < rows && start < plen && diff != 0;
    const unsigned long long mask = __ballot(bad);
    const uint32_t lane = threadIdx.x & 63u;
    if (log2_width >= 6) {
        // (rows is a multiple of 64: g < rows is wave-uniform)
        if (lane == 0 && g < rows) bad_words[((size_t)piece << (log2_width - 6)) + (slot >> 6)] = mask;
    } else if (slot == 0 && g < rows) {
        bad_words[piece] = (mask >> lane) & ((1ull << (1u << log2_width)) - 1);
    }
}

// Block stream (the re-verify from disk): lane b hashes stage
// block b, lens[b] bytes at stage + b*16 KiB, into leaf row rows[b].  A launch
// is tied to no piece and no width: the host cuts a round wherever its stage
// is full and says where each block's row lies.  lens[b] == 0 is an absent
// slot (the zero hash; its stage bytes are never read, it need not have any);
// rows[b] == kSkipRow is a hole in the stage and stores nothing.  The streaming
// is the leaf kernel's: two-group ring, wave-uniform bound, clamped loads, so
// a wave of full blocks runs the ring and the constant padding block only and
// a wave of tails skips the ring.
constexpr uint32_t kSkipRow = 0xFFFFFFFFu;

__global__ __launch_bounds__(kBlock) void merkle_block_kernel(const uint8_t* __restrict__ stage,
                                                              const uint32_t* __restrict__ rows,
                                                              const uint32_t* __restrict__ lens, uint32_t n_blocks,
                                                              uint8_t* __restrict__ leaves) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    // Lanes past the last block redo it (in bounds, the wave stays convergent)
    // and store nothing.
    const uint32_t b = g < n_blocks ? g : n_blocks - 1;
    const uint32_t row = rows[b];
    const uint32_t leaf_len = row == kSkipRow ? 0 : lens[b];
    const uint8_t* p = stage + (size_t)b * kLeaf;
    const uint32_t ng = leaf_len >> 7;
    const uint32_t ng_wave = __builtin_amdgcn_readfirstlane(wave_max(ng));
    State s = sha256::iv();
    stream_groups(s, reinterpret_cast<const uint4*>(p), ng, ng_wave);
    if (leaf_len == kLeaf) {
        sha256::compress_const(s, kPadLeaf);
    } else if (leaf_len) {
        finish_tail(s, p + (size_t)ng * 128, leaf_len & 127u, leaf_len);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) s.h[k] = 0;  // an absent slot: the zero hash, not a hash of anything
    }
    if (g < n_blocks && row != kSkipRow) store_row(leaves, row, s);
}

// Leaf check (the re-verify from disk, block by block; DESIGN.md §3.7 "Block
// checks from disk"): one launch per group of pieces a round finished, beside
// the group's node launch.  Lane g = (k << K) + slot takes row g of `window`
// (the group's first ring row; the group does not wrap): slot `slot` of piece
// k, live iff slot < blocks[k]; the piece's rows of the compact leaf table
// start at row leaf_first[k].  Nothing is hashed.
//  * leaves_out (copy-out): a live slot's window row goes to row
//    leaf_first[k] + slot.
//  * expected_leaves (check; with bad_words and shadow): the stored row
//    leaf_first[k] + slot is compared with the window row; a live slot that
//    differs is bad, a dead one never is.  The stored row (32 zero bytes for a
//    dead slot) also goes to row g of `shadow`, which the node kernels then
//    reduce as they reduce the window.
// The bitmap is merkle_block_check_kernel's, but with the caller's words per
// piece (wpp >= max(1, 2^K / 64): a group may be narrower than the call):
// K >= 6, a wave is 64 slots of one piece and lane 0 stores its word; K < 6, a
// wave holds 64 >> K whole pieces and each piece's slot-0 lane stores its 2^K
// bits.  The words of a piece that its group does not cover are not written.
// Every word has at most one writing lane (no atomics, no LDS).
__global__ __launch_bounds__(kBlock) void merkle_leaf_check_kernel(const uint8_t* __restrict__ window, uint32_t n,
                                                                   uint32_t log2_width, uint32_t wpp,
                                                                   const uint32_t* __restrict__ leaf_first,
                                                                   const uint32_t* __restrict__ blocks,
                                                                   const uint8_t* __restrict__ expected_leaves,
                                                                   unsigned long long* __restrict__ bad_words,
                                                                   uint8_t* __restrict__ shadow,
                                                                   uint8_t* __restrict__ leaves_out) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t rows = n << log2_width;
    // Lanes past the last row redo row rows-1 (in bounds, the wave stays
    // convergent), store nothing and contribute 0 to the ballot.
    const uint32_t gg = g < rows ? g : rows - 1;
    const uint32_t piece = gg >> log2_width;
    const uint32_t slot = gg & ((1u << log2_width) - 1);
    const uint32_t nb = blocks[piece];  // >= 1: a piece has a byte
    const uint32_t first = leaf_first[piece];
    const bool live = slot < nb, mine = g < rows;
    const uint4* w = reinterpret_cast<const uint4*>(window + (size_t)gg * 32);
    const uint4 w0 = w[0], w1 = w[1];
    if (leaves_out && mine && live) {
        uint4* o = reinterpret_cast<uint4*>(leaves_out + ((size_t)first + slot) * 32);
        o[0] = w0;
        o[1] = w1;
    }
    if (!expected_leaves) return;  // (kernel-uniform)
    // a dead slot loads the piece's last row (in bounds) and drops it
    const uint4* x = reinterpret_cast<const uint4*>(expected_leaves + ((size_t)first + (live ? slot : nb - 1)) * 32);
    uint4 x0 = x[0], x1 = x[1];
    if (!live) x0 = x1 = make_uint4(0, 0, 0, 0);
    const uint32_t diff = (x0.x ^ w0.x) | (x0.y ^ w0.y) | (x0.z ^ w0.z) | (x0.w ^ w0.w) | (x1.x ^ w1.x) |
                          (x1.y ^ w1.y) | (x1.z ^ w1.z) | (x1.w ^ w1.w);
    if (shadow && mine) {
        uint4* o = reinterpret_cast<uint4*>(shadow + (size_t)gg * 32);
        o[0] = x0;
        o[1] = x1;
    }
    const unsigned long long mask = __ballot(mine && live && diff != 0);
    const uint32_t lane = threadIdx.x & 63u;
    if (log2_width >= 6) {
        // (rows is a multiple of 64: g < rows is wave-uniform)
        if (lane == 0 && mine) bad_words[(size_t)piece * wpp + (slot >> 6)] = mask;
    } else if (slot == 0 && mine) {
        bad_words[(size_t)piece * wpp] = (mask >> lane) & ((1ull << (1u << log2_width)) - 1);
    }
}

// ---------------------------------------------------------------------------
// Node reduction.

// node = SHA-256(left || right); rows are big-endian bytes.
__device__ __forceinline__ void node_hash(uint4& o0, uint4& o1, const uint4& l0, const uint4& l1, const uint4& r0,
                                          const uint4& r1) {
    State s = sha256::iv();
    sha256::compress_le(s, l0, l1, r0, r1);
    sha256::compress_const(s, kPadNode);
    o0 = make_uint4(sha256::bswap(s.h[0]), sha256::bswap(s.h[1]), sha256::bswap(s.h[2]), sha256::bswap(s.h[3]));
    o1 = make_uint4(sha256::bswap(s.h[4]), sha256::bswap(s.h[5]), sha256::bswap(s.h[6]), sha256::bswap(s.h[7]));
}

// Rows in LDS as two planes of uint4 (row r = lo[r] | hi[r]): a 16-byte
// stride per lane, conflict-free ds_read_b128 / ds_write_b128.
struct Rows {
    uint4 lo[kTile];
    uint4 hi[kTile];
};

// One level in place: the first 2*count rows become count rows.  Every thread
// of the workgroup calls this (barriers inside).
template <class Tile>
__device__ __forceinline__ void reduce_level(Tile& t, uint32_t count) {
    const uint32_t i = threadIdx.x;
    uint4 o0, o1;
    if (i < count) node_hash(o0, o1, t.lo[2 * i], t.hi[2 * i], t.lo[2 * i + 1], t.hi[2 * i + 1]);
    __syncthreads();
    if (i < count) {
        t.lo[i] = o0;
        t.hi[i] = o1;
    }
    __syncthreads();
}

struct Row {
    uint4 lo, hi;
};

__device__ __forceinline__ void emit_root(const Row& r, uint32_t piece, uint8_t* __restrict__ roots,
                                          const uint8_t* __restrict__ expected, uint8_t* __restrict__ matched) {
    if (roots) {
        uint4* o = reinterpret_cast<uint4*>(roots + (size_t)piece * 32);
        o[0] = r.lo;
        o[1] = r.hi;
    }
    if (expected && matched) {
        const uint32_t* x = reinterpret_cast<const uint32_t*>(expected + (size_t)piece * 32);  // 4-byte aligned
        const bool ok = (x[0] == r.lo.x) & (x[1] == r.lo.y) & (x[2] == r.lo.z) & (x[3] == r.lo.w) &
                        (x[4] == r.hi.x) & (x[5] == r.hi.y) & (x[6] == r.hi.z) & (x[7] == r.hi.w);
        matched[piece] = ok ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// Fused piece kernel (the async download path): the leaf
// kernel's lanes, but a workgroup keeps its 256 leaf rows in LDS and reduces
// them there, so no leaf row reaches HBM and a batch of trees of at most 256
// leaves is one launch.
//  * log2_width <= kPieceTileLog2: a workgroup holds 256 >> log2_width whole
//    pieces; after level L every piece with log2w == L emits its root.
//  * wider: a workgroup is one 256-leaf tile of one piece and stores the
//    tile's top (row 0 after min(log2w, 8) levels) to tops[(piece <<
//    (log2_width - 8)) + tile], for the tiles under the piece's own root only;
//    tile 0 also stores log2w_top[piece] = max(log2w - 8, 0).  The host then
//    runs the node kernel over tops at width log2_width - 8: the kernel
//    boundary is what orders the tops between workgroups.
constexpr int kPieceTileLog2 = 8;
static_assert((1 << kPieceTileLog2) == kBlock, "one leaf per thread of the workgroup");

struct PieceRows {
    uint4 lo[kBlock];
    uint4 hi[kBlock];
};

// The tree phase of the piece kernels: the workgroup's 256 leaf rows are in t
// (a barrier behind the last write); every thread of the workgroup calls this.
__device__ __forceinline__ void piece_tree_phase(PieceRows& t, const uint8_t* __restrict__ log2w, uint32_t n,
                                                 uint32_t log2_width, uint8_t* __restrict__ tops,
                                                 uint8_t* __restrict__ log2w_top, uint8_t* __restrict__ roots,
                                                 const uint8_t* __restrict__ expected, uint8_t* __restrict__ matched) {
    const uint32_t i = threadIdx.x;
    if (log2_width <= (uint32_t)kPieceTileLog2) {
        const uint32_t per = (uint32_t)kBlock >> log2_width;  // pieces of this workgroup: one thread each
        const uint32_t piece = blockIdx.x * per + i;
        const bool mine = i < per && piece < n;
        const uint32_t want = mine ? (log2w ? log2w[piece] : log2_width) : 0xFFFFFFFFu;
        for (uint32_t L = 0;; ++L) {
            if (want == L)
                emit_root(Row{t.lo[(i << log2_width) >> L], t.hi[(i << log2_width) >> L]}, piece, roots, expected,
                          matched);
            if (L == log2_width) break;
            reduce_level(t, (uint32_t)kBlock >> (L + 1));
        }
    } else {
        const uint32_t tshift = log2_width - kPieceTileLog2;
        const uint32_t piece = blockIdx.x >> tshift;  // (< n: n << log2_width rows are whole tiles)
        const uint32_t tile = blockIdx.x & ((1u << tshift) - 1);
        const uint32_t want = log2w ? log2w[piece] : log2_width;  // (workgroup-uniform)
        const uint32_t levels = want < (uint32_t)kPieceTileLog2 ? want : (uint32_t)kPieceTileLog2;
        // (a log2w above log2_width is not a level of this tree: clamped, it stays in bounds and emits nothing)
        const uint32_t want_top = want - levels < tshift + 1 ? want - levels : tshift + 1;
        for (uint32_t L = 0; L < levels; ++L) reduce_level(t, (uint32_t)kBlock >> (L + 1));
        if (i == 0 && tile < (1u << want_top)) {
            uint4* o = reinterpret_cast<uint4*>(tops + ((size_t)(piece << tshift) + tile) * 32);
            o[0] = t.lo[0];
            o[1] = t.hi[0];
            if (tile == 0) log2w_top[piece] = (uint8_t)want_top;
        }
    }
}

__global__ __launch_bounds__(kBlock) void merkle_piece_kernel(const uint8_t* __restrict__ base,
                                                              const uint64_t* __restrict__ offsets,
                                                              const uint32_t* __restrict__ lens,
                                                              const uint8_t* __restrict__ log2w, uint32_t n,
                                                              uint32_t log2_width, uint8_t* __restrict__ tops,
                                                              uint8_t* __restrict__ log2w_top,
                                                              uint8_t* __restrict__ roots,
                                                              const uint8_t* __restrict__ expected,
                                                              uint8_t* __restrict__ matched) {
    __shared__ PieceRows t;
    const uint32_t i = threadIdx.x;
    {
        // the leaf phase, as merkle_leaf_kernel<true>
        const uint32_t g = blockIdx.x * kBlock + i;
        const uint32_t rows = n << log2_width;
        // Lanes past the last row redo row rows-1 (in bounds, the wave stays
        // convergent); their LDS rows belong to pieces >= n and are never emitted.
        const uint32_t gg = g < rows ? g : rows - 1;
        const uint32_t piece = gg >> log2_width;
        const uint32_t slot = gg & ((1u << log2_width) - 1);
        const uint32_t plen = lens[piece];
        const uint8_t* p = base + offsets[piece];
        const uint64_t start = (uint64_t)slot * kLeaf;
        const uint32_t leaf_len = start < plen ? (plen - start < kLeaf ? (uint32_t)(plen - start) : kLeaf) : 0;
        const uint32_t ng = leaf_len >> 7;
        const uint32_t ng_wave = __builtin_amdgcn_readfirstlane(wave_max(ng));
        p += start < plen ? start : 0;
        State s = sha256::iv();
        stream_groups(s, reinterpret_cast<const uint4*>(p), ng, ng_wave);
        if (leaf_len == kLeaf) {
            sha256::compress_const(s, kPadLeaf);
        } else if (leaf_len) {
            finish_tail(s, p + (size_t)ng * 128, leaf_len & 127u, leaf_len);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) s.h[k] = 0;  // beyond the piece: the zero hash, not a hash of anything
        }
        t.lo[i] = make_uint4(sha256::bswap(s.h[0]), sha256::bswap(s.h[1]), sha256::bswap(s.h[2]), sha256::bswap(s.h[3]));
        t.hi[i] = make_uint4(sha256::bswap(s.h[4]), sha256::bswap(s.h[5]), sha256::bswap(s.h[6]), sha256::bswap(s.h[7]));
    }
    __syncthreads();
    piece_tree_phase(t, log2w, n, log2_width, tops, log2w_top, roots, expected, matched);
}

// ---------------------------------------------------------------------------
// Zero-copy piece kernel (vx_set_merkle_zero_copy):
// merkle_piece_kernel with piece i at the device-visible address srcs[i] (HBM,
// or a registered host buffer's mapping; 16-byte aligned) instead of base +
// offsets[i], so a v2 slot's PCIe transfer overlaps its own hashing.  Thread i
// of a workgroup still owns leaf row i of the workgroup's 256 and the tree
// phase is piece_tree_phase; only the leaf phase differs.  Over PCIe the load
// shape decides the rate (sha1_zc_split_kernel's comment): one lane streaming
// its own leaf reaches 28-31 GiB/s, so the loads are cooperative.
//  * A wave serves its own 64 leaves.  A tile is kZcTileBytes = 256 contiguous
//    bytes of each of them: 16 wave instructions, each 16 lanes x 16 bytes on
//    each of 4 leaves (the shape §6.5 measured), 16 KiB per wave and tile.
//  * kZcInFlight = 2 tiles are in flight per wave in two register tiles (ra,
//    rb): while tile t is hashed, t + 1 and t + 2 are on the wire, 32 KiB per
//    wave, 128 KiB per workgroup, so a slot of 8 workgroups or more (2,048
//    leaves: 32 pieces of 1 MiB) has the ~1 MiB in flight that the SHA-1
//    kernel needed to reach the copy rate.
//  * A landed tile is transposed through the wave's own LDS stage (chunk c of
//    leaf l at [c][l], rows padded to 65 slots: lane-linear reads, and writes
//    that spread a 16-lane group over all banks) to the lane that owns the
//    leaf, which compresses its four 64-byte blocks.  There is no chain
//    between leaves, so a wave stages and hashes for itself: LDS executes a
//    wave's accesses in order, and wavefront-scope fences keep the compiler
//    from moving them; no workgroup barrier before the tree phase.
//  * The loop bound is the wave's largest tile count.  A load whose leaf has no
//    full tile left (t >= leaf_len >> 8; every lane of a tile of the prefetch
//    past the end) reads the device zero line, so no cooperative load touches a
//    byte at or past the end of a leaf's last full tile.  The < 256 bytes
//    behind it are the owning lane's (finish_tail: byte-exact, the padding from
//    those bytes only); a leaf slot at or past the piece's end (a piece of 0
//    bytes: every slot) and a lane past the launch's rows read nothing and give
//    the zero row.
constexpr uint32_t kZcLeavesPerWave = 64;
constexpr uint32_t kZcTileBytes = 256;                  // bytes per leaf per tile
constexpr uint32_t kZcTileChunks = kZcTileBytes / 16;   // 16-byte chunks per leaf per tile = wave instructions per tile
constexpr uint32_t kZcInFlight = 2;                     // register tiles per wave
constexpr uint32_t kZcStageRow = kZcLeavesPerWave + 1;  // padded
static_assert(kZcLeavesPerWave == 64 && kZcTileChunks == 16, "an instruction is 16 lanes on each of 4 leaves");

typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) U32x4 GlobalU32x4;

struct ZcStage {
    uint4 c[kBlock / 64][kZcTileChunks][kZcStageRow];
};
constexpr uint32_t kZcLdsBytes = sizeof(ZcStage) + sizeof(PieceRows);
static_assert(2 * kZcLdsBytes <= 160 * 1024, "two workgroups per CU");

// This lane's 16 loads of tile t: instruction k moves chunk lane & 15 of leaf
// 4k + (lane >> 4).  zb[k]: that chunk's address in tile 0, zn[k]: the leaf's
// full tiles.  Explicitly global vector loads, as zc_load of the SHA-1 kernel.
__device__ __forceinline__ void zc_leaf_tile(uint4 (&r)[kZcTileChunks], const uint64_t (&zb)[kZcTileChunks],
                                             const uint32_t (&zn)[kZcTileChunks], uint32_t t) {
    const uint64_t zero = reinterpret_cast<uint64_t>(g_zero_group);
#pragma unroll
    for (uint32_t k = 0; k < kZcTileChunks; ++k) {
        const uint64_t a = t < zn[k] ? zb[k] + (uint64_t)t * kZcTileBytes : zero;
        const U32x4 v = *reinterpret_cast<GlobalU32x4*>(a);
        r[k] = make_uint4(v.x, v.y, v.z, v.w);
    }
}

// Tile t (landed in r) through the wave's stage into the owning lanes' states,
// r refilled with tile t_next behind the stage writes.
__device__ __forceinline__ void zc_leaf_step(State& s, uint4 (&r)[kZcTileChunks], uint4 (&st)[kZcTileChunks][kZcStageRow],
                                             const uint64_t (&zb)[kZcTileChunks], const uint32_t (&zn)[kZcTileChunks],
                                             uint32_t t, uint32_t t_next, uint32_t nt, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 0; k < kZcTileChunks; ++k) st[lane & 15][4 * k + (lane >> 4)] = r[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    zc_leaf_tile(r, zb, zn, t_next);
    if (t < nt) {
#pragma unroll
        for (uint32_t b = 0; b < kZcTileChunks / 4; ++b)
            sha256::compress_le(s, st[4 * b][lane], st[4 * b + 1][lane], st[4 * b + 2][lane], st[4 * b + 3][lane]);
    }
    // the stage is read before the next tile's writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBlock) void merkle_zc_piece_kernel(const uint64_t* __restrict__ srcs,
                                                                 const uint32_t* __restrict__ lens,
                                                                 const uint8_t* __restrict__ log2w, uint32_t n,
                                                                 uint32_t log2_width, uint8_t* __restrict__ tops,
                                                                 uint8_t* __restrict__ log2w_top,
                                                                 uint8_t* __restrict__ roots,
                                                                 const uint8_t* __restrict__ expected,
                                                                 uint8_t* __restrict__ matched) {
    __shared__ PieceRows t;
    __shared__ ZcStage stage;
    const uint32_t i = threadIdx.x;
    {
        const uint32_t lane = i & 63u;
        const uint32_t wave = __builtin_amdgcn_readfirstlane(i >> 6);
        const uint32_t g = blockIdx.x * kBlock + i;
        const uint32_t rows = n << log2_width;
        // Lanes past the last row read their tables at row rows-1 (in bounds) and hash nothing;
        // their LDS rows belong to pieces >= n and are never emitted.
        const uint32_t gg = g < rows ? g : rows - 1;
        const uint32_t piece = gg >> log2_width;
        const uint32_t slot = gg & ((1u << log2_width) - 1);
        const uint32_t plen = lens[piece];
        const uint64_t start = (uint64_t)slot * kLeaf;
        const uint32_t leaf_len =
            g < rows && start < plen ? (plen - start < kLeaf ? (uint32_t)(plen - start) : kLeaf) : 0;
        const uint64_t p = srcs[piece] + (leaf_len ? start : 0);  // (not an address of anything when leaf_len == 0)
        const uint32_t nt = leaf_len / kZcTileBytes;
        const uint32_t nt_wave = __builtin_amdgcn_readfirstlane(wave_max(nt));
        State s = sha256::iv();
        if (nt_wave) {  // (wave-uniform)
            uint64_t zb[kZcTileChunks];
            uint32_t zn[kZcTileChunks];
#pragma unroll
            for (uint32_t k = 0; k < kZcTileChunks; ++k) {
                const int l = (int)(4 * k + (lane >> 4));
                const uint32_t lo = __shfl((uint32_t)p, l, 64), hi = __shfl((uint32_t)(p >> 32), l, 64);
                zb[k] = (((uint64_t)hi << 32) | lo) + 16u * (lane & 15u);
                zn[k] = __shfl(nt, l, 64);
            }
            uint4 ra[kZcTileChunks], rb[kZcTileChunks];
            zc_leaf_tile(ra, zb, zn, 0);
            zc_leaf_tile(rb, zb, zn, 1);
            for (uint32_t t0 = 0; t0 < nt_wave; t0 += kZcInFlight) {
                zc_leaf_step(s, ra, stage.c[wave], zb, zn, t0, t0 + 2, nt, lane);
                zc_leaf_step(s, rb, stage.c[wave], zb, zn, t0 + 1, t0 + 3, nt, lane);
            }
        }
        if (leaf_len == kLeaf) {
            sha256::compress_const(s, kPadLeaf);
        } else if (leaf_len) {
            finish_tail(s, reinterpret_cast<const uint8_t*>(p + (uint64_t)nt * kZcTileBytes),
                        leaf_len % kZcTileBytes, leaf_len);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) s.h[k] = 0;  // beyond the piece: the zero hash, not a hash of anything
        }
        t.lo[i] = make_uint4(sha256::bswap(s.h[0]), sha256::bswap(s.h[1]), sha256::bswap(s.h[2]), sha256::bswap(s.h[3]));
        t.hi[i] = make_uint4(sha256::bswap(s.h[4]), sha256::bswap(s.h[5]), sha256::bswap(s.h[6]), sha256::bswap(s.h[7]));
    }
    __syncthreads();
    piece_tree_phase(t, log2w, n, log2_width, tops, log2w_top, roots, expected, matched);
}

// Trees of at most kTile leaves: workgroup b reduces rows [b*kTile, +kTile) =
// pieces [b*P, +P), P = kTile >> log2_width.  After level L the root of a
// piece with log2w == L is row (piece's first row) >> L.
__global__ __launch_bounds__(kNodeBlock) void merkle_node_kernel(const uint8_t* __restrict__ leaves, uint32_t n,
                                                                 uint32_t log2_width,
                                                                 const uint8_t* __restrict__ log2w,
                                                                 uint8_t* __restrict__ roots,
                                                                 const uint8_t* __restrict__ expected,
                                                                 uint8_t* __restrict__ matched) {
    __shared__ Rows t;
    const uint32_t i = threadIdx.x;
    const uint32_t rows = n << log2_width;
    const uint32_t row0 = blockIdx.x * kTile;
    const uint4* src = reinterpret_cast<const uint4*>(leaves);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t r = i + k * kNodeBlock;
        const bool in = row0 + r < rows;  // (row0 + r < 2^32: rows fits 32 bits and kTile divides the grid's span)
        t.lo[r] = in ? src[(size_t)(row0 + r) * 2] : make_uint4(0, 0, 0, 0);
        t.hi[r] = in ? src[(size_t)(row0 + r) * 2 + 1] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    // pieces of this tile: up to kTile of them (log2_width 0), so a thread may own two
    const uint32_t per = kTile >> log2_width;
    for (uint32_t L = 0;; ++L) {
        for (uint32_t q = i; q < per; q += kNodeBlock) {
            const uint32_t piece = blockIdx.x * per + q;
            if (piece < n && (log2w ? log2w[piece] : log2_width) == L)
                emit_root(Row{t.lo[(q << log2_width) >> L], t.hi[(q << log2_width) >> L]}, piece, roots, expected,
                          matched);
        }
        if (L == log2_width) break;
        reduce_level(t, kTile >> (L + 1));
    }
}

// Trees wider than a tile: one workgroup per piece.  Each tile of kTile leaves
// is reduced to its top, the tops (at most kMaxTops) are reduced in turn.  A
// piece's own log2w picks its root from the first tile (log2w <= kTileLog2) or
// from the tops.
__global__ __launch_bounds__(kNodeBlock) void merkle_wide_node_kernel(const uint8_t* __restrict__ leaves,
                                                                      uint32_t log2_width,
                                                                      const uint8_t* __restrict__ log2w,
                                                                      uint8_t* __restrict__ roots,
                                                                      const uint8_t* __restrict__ expected,
                                                                      uint8_t* __restrict__ matched) {
    __shared__ Rows t;
    __shared__ uint4 top_lo[kMaxTops], top_hi[kMaxTops];
    const uint32_t i = threadIdx.x;
    const uint32_t piece = blockIdx.x;
    const uint32_t want = log2w ? log2w[piece] : log2_width;
    // the tiles under the piece's own root (workgroup-uniform)
    const uint32_t ntiles = want <= (uint32_t)kTileLog2 ? 1u : 1u << (want - kTileLog2);
    if (want > log2_width) return;  // not a level of this tree: nothing to emit
    const uint4* src = reinterpret_cast<const uint4*>(leaves) + ((size_t)piece << log2_width) * 2;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t r = i + k * kNodeBlock;
            t.lo[r] = src[((size_t)tile * kTile + r) * 2];
            t.hi[r] = src[((size_t)tile * kTile + r) * 2 + 1];
        }
        __syncthreads();
        for (uint32_t L = 0;; ++L) {
            if (tile == 0 && want == L && i == 0) emit_root(Row{t.lo[0], t.hi[0]}, piece, roots, expected, matched);
            if (L == kTileLog2) break;
            reduce_level(t, kTile >> (L + 1));
        }
        if (i == 0) {
            top_lo[tile] = t.lo[0];
            top_hi[tile] = t.hi[0];
        }
        __syncthreads();
    }
    if (want <= kTileLog2) return;  // (workgroup-uniform)
    for (uint32_t k = i; k < ntiles; k += kNodeBlock) {
        t.lo[k] = top_lo[k];
        t.hi[k] = top_hi[k];
    }
    __syncthreads();
    for (uint32_t L = kTileLog2 + 1; L <= want; ++L) reduce_level(t, (1u << want) >> L);
    if (i == 0) emit_root(Row{t.lo[0], t.hi[0]}, piece, roots, expected, matched);
}

// One pass of a layer reduction: workgroup b reduces rows [b << levels,
// +(1 << levels)) of the m-row input to output row b; rows at or past m are
// the pad hash of the input's height.  levels <= kTileLog2.
__global__ __launch_bounds__(kNodeBlock) void merkle_layer_kernel(const uint8_t* __restrict__ in, uint32_t m,
                                                                  uint32_t levels, uint4 pad_lo, uint4 pad_hi,
                                                                  uint8_t* __restrict__ out) {
    __shared__ Rows t;
    const uint32_t i = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x << levels;
    const uint4* src = reinterpret_cast<const uint4*>(in);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t r = i + k * kNodeBlock;
        const bool in_layer = row0 + r < m;
        t.lo[r] = in_layer ? src[(row0 + r) * 2] : pad_lo;
        t.hi[r] = in_layer ? src[(row0 + r) * 2 + 1] : pad_hi;
    }
    __syncthreads();
    for (uint32_t L = 0; L < levels; ++L) reduce_level(t, (1u << levels) >> (L + 1));
    if (i == 0) {
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)blockIdx.x * 32);
        o[0] = t.lo[0];
        o[1] = t.hi[0];
    }
}

// c ? a : b by value, word by word.  (?: on two uint4 lvalues selects between
// their addresses, which puts a local one into scratch.)
__device__ __forceinline__ uint4 pick(bool c, const uint4 a, const uint4 b) {
    return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// Rows [row0, row0 + rows) of src into the tile, the rest of it filled with the
// pad row.  rows <= kTile; every thread of the workgroup calls this (a barrier
// at the end).
__device__ __forceinline__ void load_rows(Rows& t, const uint4* src, uint64_t row0, uint32_t rows, const uint4 pad_lo,
                                          const uint4 pad_hi) {
    const uint32_t i = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t r = i + k * kNodeBlock;
        uint4 lo = pad_lo, hi = pad_hi;
        if (r < rows) {
            lo = src[(row0 + r) * 2];
            hi = src[(row0 + r) * 2 + 1];
        }
        t.lo[r] = lo;
        t.hi[r] = hi;
    }
    __syncthreads();
}

// The tile reduction of the layers and proofs kernels: rows [row0, row0 + rows)
// of src, filled to 1 << levels with the pad row, reduced to t row 0.  rows <=
// kTile, levels <= kTileLog2; every thread of the workgroup calls this.
__device__ __forceinline__ void reduce_rows(Rows& t, const uint4* src, uint64_t row0, uint32_t rows, uint32_t levels,
                                            const uint4 pad_lo, const uint4 pad_hi) {
    load_rows(t, src, row0, rows, pad_lo, pad_hi);
    for (uint32_t L = 0; L < levels; ++L) reduce_level(t, (1u << levels) >> (L + 1));
}

// One pass of the segmented layer reduction (vx_merkle_device_layers): workgroup
// b executes tile tiles[b] of the host's plan (vx_merkle_layers.hpp).  The
// descriptor's address is workgroup-uniform, so it is fetched once per wave
// with scalar loads.  in: d_hashes in pass 0, the work area later; a tile that
// is not its layer's last writes a work row that only the next launch reads.
__global__ __launch_bounds__(kNodeBlock) void merkle_layers_kernel(const uint8_t* in,
                                                                   const vx_merkle_tile* __restrict__ tiles,
                                                                   uint4 pad_lo, uint4 pad_hi, uint8_t* work,
                                                                   uint8_t* __restrict__ roots,
                                                                   const uint8_t* __restrict__ expected,
                                                                   uint8_t* __restrict__ matched) {
    __shared__ Rows t;
    // (as words: the 16- and 8-bit fields have no scalar load of their own)
    const uint32_t* d = reinterpret_cast<const uint32_t*>(tiles + blockIdx.x);
    const uint32_t in_row = d[0], out = d[1], packed = d[2];  // rows | levels << 16 | last << 24
    const uint32_t d_rows = packed & 0xFFFFu, d_levels = (packed >> 16) & 0xFFu, last = packed >> 24;
    // (a plan is the host's own, but a clamp costs nothing and keeps the tile inside LDS whatever it holds)
    const uint32_t rows = d_rows < kTile ? d_rows : kTile;
    const uint32_t levels = d_levels < (uint32_t)kTileLog2 ? d_levels : (uint32_t)kTileLog2;
    reduce_rows(t, reinterpret_cast<const uint4*>(in), in_row, rows, levels, pad_lo, pad_hi);
    if (threadIdx.x == 0) {
        if (last) {
            emit_root(Row{t.lo[0], t.hi[0]}, out, roots, expected, matched);
        } else {
            uint4* o = reinterpret_cast<uint4*>(work + (size_t)out * 32);
            o[0] = t.lo[0];
            o[1] = t.hi[0];
        }
    }
}

// Rows [0, count) of the LDS tile to tree rows [row0, row0 + count): lane l of a
// step stores uint4 l of the run (row l / 2, its low or high half), so a wave
// writes 1 KiB of consecutive bytes.  The caller has a barrier behind the
// tile's last write; the tile is only read here.
__device__ __forceinline__ void store_rows(const Rows& t, uint8_t* tree, uint64_t row0, uint32_t count) {
    uint4* dst = reinterpret_cast<uint4*>(tree) + row0 * 2;
    for (uint32_t u = threadIdx.x; u < 2 * count; u += kNodeBlock) dst[u] = (u & 1) ? t.hi[u >> 1] : t.lo[u >> 1];
}

// One pass of the layer trees (vx_merkle_device_trees): workgroup b executes
// tile tiles[b] of the host's plan (vx_merkle_tree.hpp).  The tile is rows
// [512 * tile, +rows) of a level of level_rows rows; it is loaded as
// reduce_rows loads it, the rest filled with the pass's pad hash, and after
// each level of the reduction the rows of that level that exist,
// ceil(rows / 2^j), go to their place in the tree: the next level starts
// level_rows rows further on and is half as long, and the tile's rows start at
// half the position.  in: d_hashes in pass 0 (copy0 set: the loaded rows are
// also stored, as level 0 of the tree), the tree itself later; a later pass
// reads level 9p only, which the launch before it wrote, and writes the levels
// above it.  rows and levels are not taken from the descriptor but follow from
// level_rows and tile, so whatever the descriptor holds the tile stays inside
// LDS (the clamp of merkle_layers_kernel).
__global__ __launch_bounds__(kNodeBlock) void merkle_tree_kernel(const uint8_t* in,
                                                                 const vx_merkle_tree_tile* __restrict__ tiles,
                                                                 uint4 pad_lo, uint4 pad_hi, uint32_t copy0,
                                                                 uint8_t* tree) {
    __shared__ Rows t;
    const uint32_t* d = reinterpret_cast<const uint32_t*>(tiles + blockIdx.x);  // (workgroup-uniform: scalar loads)
    const uint32_t src_row = d[0], dst_row = d[1], level_rows = d[2], tile = d[3];
    uint64_t pos = (uint64_t)tile << kTileLog2;
    const uint64_t left = pos < level_rows ? level_rows - pos : 0;
    const uint32_t rows = left < kTile ? (uint32_t)left : kTile;
    uint32_t levels = kTileLog2;
    if (level_rows <= kTile) levels = level_rows > 1 ? 32u - (uint32_t)__builtin_clz(level_rows - 1) : 0;
    load_rows(t, reinterpret_cast<const uint4*>(in), (uint64_t)src_row + pos, rows, pad_lo, pad_hi);
    uint64_t base = dst_row, n = level_rows;
    if (copy0) store_rows(t, tree, base + pos, rows);
    for (uint32_t j = 1; j <= levels; ++j) {
        reduce_level(t, (1u << levels) >> j);
        base += n;
        n = (n + 1) >> 1;
        pos >>= 1;
        store_rows(t, tree, base + pos, (rows + (1u << j) - 1) >> j);
    }
}

static_assert(sizeof(vx_merkle_tree_tile) == 16 && offsetof(vx_merkle_tree_tile, dst_row) == 4 &&
                  offsetof(vx_merkle_tree_tile, level_rows) == 8 && offsetof(vx_merkle_tree_tile, tile) == 12,
              "merkle_tree_kernel reads the descriptor as words");
static_assert(sizeof(vx_merkle_tile) == 16 && offsetof(vx_merkle_tile, rows) == 8 &&
                  offsetof(vx_merkle_tile, levels) == 10 && offsetof(vx_merkle_tile, last) == 11,
              "merkle_layers_kernel reads the descriptor as words");
static_assert(sizeof(vx_merkle_proof) == 24 && offsetof(vx_merkle_proof, row) == 8 &&
                  offsetof(vx_merkle_proof, span) == 16 && offsetof(vx_merkle_proof, uncles) == 18,
              "merkle_proof_span_kernel reads the descriptor as words");

// Hash proofs (vx_merkle_device_proofs).  A descriptor comes off the wire, so
// both kernels check it before any row of the proof is read.
__device__ __forceinline__ bool proof_ok(uint32_t span, uint32_t uncles) {
    return span >= 1 && span <= kTile && (span & (span - 1)) == 0 && uncles <= 64;
}

// First launch: workgroup b reduces the span of proof b (span rows from row
// p.row of hashes) to its root in tops row b; a span of 1 is a copy.  A bad
// descriptor gets the zero row.
__global__ __launch_bounds__(kNodeBlock) void merkle_proof_span_kernel(const uint8_t* __restrict__ hashes,
                                                                       const vx_merkle_proof* __restrict__ proofs,
                                                                       uint8_t* __restrict__ tops) {
    __shared__ Rows t;
    // (as words: a copy of the struct, with its byte array, would live in scratch,
    // and the 16- and 8-bit fields have no scalar load of their own)
    const uint32_t* d = reinterpret_cast<const uint32_t*>(proofs + blockIdx.x);
    const uint32_t row = d[2], span = d[4] & 0xFFFFu, uncles = (d[4] >> 16) & 0xFFu;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4* o = reinterpret_cast<uint4*>(tops + (size_t)blockIdx.x * 32);
    if (!proof_ok(span, uncles)) {  // (workgroup-uniform)
        if (threadIdx.x == 0) {
            o[0] = zero;
            o[1] = zero;
        }
        return;
    }
    const uint32_t levels = 31u - (uint32_t)__builtin_clz(span);
    reduce_rows(t, reinterpret_cast<const uint4*>(hashes), row, span, levels, zero, zero);
    if (threadIdx.x == 0) {
        o[0] = t.lo[0];
        o[1] = t.hi[0];
    }
}

// Second launch: lane g walks proof g's uncles from the span's root in tops
// row g (the first launch's), leaves the top there and sets the verdict.  The
// loop bound is the wave's largest uncle count; a lane past its own count
// loads nothing and keeps its hash (as the leaf kernels treat group counts).
__global__ __launch_bounds__(kBlock) void merkle_proof_walk_kernel(const uint8_t* __restrict__ hashes,
                                                                   const vx_merkle_proof* __restrict__ proofs,
                                                                   uint32_t n, uint8_t* tops,
                                                                   const uint8_t* __restrict__ expected,
                                                                   uint8_t* __restrict__ matched) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    // Lanes past the last proof redo it (in bounds, the wave stays convergent) and store nothing.
    const vx_merkle_proof* p = proofs + (g < n ? g : n - 1);
    const uint32_t span = p->span, uncles = p->uncles, row = p->row;
    const uint64_t pos = p->pos;
    const bool ok = proof_ok(span, uncles);
    const uint32_t un = ok && g < n ? uncles : 0;
    const uint32_t un_wave = __builtin_amdgcn_readfirstlane(wave_max(un));
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4* top = reinterpret_cast<uint4*>(tops) + (size_t)(g < n ? g : n - 1) * 2;
    const uint4* uncle = reinterpret_cast<const uint4*>(hashes) + ((uint64_t)row + span) * 2;
    uint4 c0 = zero, c1 = zero;
    if (g < n) {
        c0 = top[0];
        c1 = top[1];
    }
    for (uint32_t k = 0; k < un_wave; ++k) {
        const bool on = k < un;
        uint4 u0 = zero, u1 = zero;
        if (on) {
            u0 = uncle[2 * k];
            u1 = uncle[2 * k + 1];
        }
        const bool right = (pos >> k) & 1;  // (k < 64)
        uint4 o0, o1;
        node_hash(o0, o1, pick(right, u0, c0), pick(right, u1, c1), pick(right, c0, u0), pick(right, c1, u1));
        c0 = pick(on, o0, c0);
        c1 = pick(on, o1, c1);
    }
    if (g >= n) return;
    if (!ok) {
        top[0] = zero;
        top[1] = zero;
        matched[g] = 0;
        return;
    }
    top[0] = c0;
    top[1] = c1;
    const uint32_t* x = reinterpret_cast<const uint32_t*>(expected + (size_t)p->expected * 32);  // 4-byte aligned
    const bool same = (x[0] == c0.x) & (x[1] == c0.y) & (x[2] == c0.z) & (x[3] == c0.w) & (x[4] == c1.x) &
                      (x[5] == c1.y) & (x[6] == c1.z) & (x[7] == c1.w);
    matched[g] = same ? 1 : 0;
}

hipError_t launch_nodes(uint32_t n, uint32_t log2_width, const uint8_t* leaves, const uint8_t* log2w, uint8_t* roots,
                        const uint8_t* expected, uint8_t* matched, hipStream_t stream) {
    if (!roots && !(expected && matched)) return hipSuccess;
    if (log2_width <= (uint32_t)kTileLog2) {
        const uint64_t rows = (uint64_t)n << log2_width;
        const uint32_t grid = (uint32_t)((rows + kTile - 1) / kTile);
        hipLaunchKernelGGL(merkle_node_kernel, dim3(grid), dim3(kNodeBlock), 0, stream, leaves, n, log2_width, log2w,
                           roots, expected, matched);
    } else {
        hipLaunchKernelGGL(merkle_wide_node_kernel, dim3(n), dim3(kNodeBlock), 0, stream, leaves, log2_width, log2w,
                           roots, expected, matched);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_merkle_uniform(const uint8_t* base, uint64_t stride, uint32_t len, uint32_t last_len, uint32_t n,
                                 uint32_t log2_width, uint8_t* leaves, uint8_t* roots, const uint8_t* expected,
                                 uint8_t* matched, hipStream_t stream) {
    const uint64_t rows = (uint64_t)n << log2_width;
    const uint32_t grid = (uint32_t)((rows + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_leaf_kernel<false>, dim3(grid), dim3(kBlock), 0, stream, base, stride, len, last_len,
                       (const uint64_t*)nullptr, (const uint32_t*)nullptr, n, log2_width, leaves);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_nodes(n, log2_width, leaves, nullptr, roots, expected, matched, stream);
}

hipError_t launch_merkle_ragged(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens,
                                const uint8_t* log2w, uint32_t n, uint32_t log2_width, uint8_t* leaves,
                                uint8_t* roots, const uint8_t* expected, uint8_t* matched, hipStream_t stream) {
    const uint64_t rows = (uint64_t)n << log2_width;
    const uint32_t grid = (uint32_t)((rows + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_leaf_kernel<true>, dim3(grid), dim3(kBlock), 0, stream, base, (uint64_t)0, 0u, 0u,
                       offsets, lens, n, log2_width, leaves);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_nodes(n, log2_width, leaves, log2w, roots, expected, matched, stream);
}

hipError_t launch_merkle_pieces(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens,
                                const uint8_t* log2w, uint32_t n, uint32_t log2_width, uint8_t* work, uint8_t* roots,
                                const uint8_t* expected, uint8_t* matched, hipStream_t stream) {
    if (!roots && !(expected && matched)) return hipSuccess;
    const uint64_t rows = (uint64_t)n << log2_width;
    const uint32_t grid = (uint32_t)((rows + kBlock - 1) / kBlock);
    const bool wide = log2_width > (uint32_t)kPieceTileLog2;
    const uint32_t top_width = wide ? log2_width - kPieceTileLog2 : 0;
    uint8_t* log2w_top = wide ? work + ((size_t)n << top_width) * 32 : nullptr;
    hipLaunchKernelGGL(merkle_piece_kernel, dim3(grid), dim3(kBlock), 0, stream, base, offsets, lens, log2w, n,
                       log2_width, wide ? work : nullptr, log2w_top, roots, expected, matched);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !wide) return e;
    return launch_nodes(n, top_width, work, log2w_top, roots, expected, matched, stream);
}

hipError_t launch_merkle_zc_pieces(const uint64_t* srcs, const uint32_t* lens, const uint8_t* log2w, uint32_t n,
                                   uint32_t log2_width, uint8_t* work, uint8_t* roots, const uint8_t* expected,
                                   uint8_t* matched, hipStream_t stream) {
    if (n == 0 || (!roots && !(expected && matched))) return hipSuccess;
    const uint64_t rows = (uint64_t)n << log2_width;
    const uint32_t grid = (uint32_t)((rows + kBlock - 1) / kBlock);
    const bool wide = log2_width > (uint32_t)kPieceTileLog2;
    const uint32_t top_width = wide ? log2_width - kPieceTileLog2 : 0;
    uint8_t* log2w_top = wide ? work + ((size_t)n << top_width) * 32 : nullptr;
    hipLaunchKernelGGL(merkle_zc_piece_kernel, dim3(grid), dim3(kBlock), 0, stream, srcs, lens, log2w, n, log2_width,
                       wide ? work : nullptr, log2w_top, roots, expected, matched);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !wide) return e;
    return launch_nodes(n, top_width, work, log2w_top, roots, expected, matched, stream);
}

void merkle_zc_geometry(uint32_t out[4]) {
    out[0] = kBlock;
    out[1] = kZcLeavesPerWave;
    out[2] = kZcTileBytes;
    out[3] = kZcInFlight;
}

hipError_t launch_merkle_block_check(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens, uint32_t n,
                                     uint32_t log2_width, const uint8_t* expected_leaves, uint64_t* bad,
                                     uint8_t* leaves_out, hipStream_t stream) {
    const uint64_t rows = (uint64_t)n << log2_width;
    const uint32_t grid = (uint32_t)((rows + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_block_check_kernel, dim3(grid), dim3(kBlock), 0, stream, base, offsets, lens, n,
                       log2_width, expected_leaves, reinterpret_cast<unsigned long long*>(bad), leaves_out);
    return hipGetLastError();
}

hipError_t launch_merkle_blocks(const uint8_t* stage, const uint32_t* rows, const uint32_t* lens, uint32_t n_blocks,
                                uint8_t* leaves, hipStream_t stream) {
    const uint32_t grid = (uint32_t)(((uint64_t)n_blocks + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_block_kernel, dim3(grid), dim3(kBlock), 0, stream, stage, rows, lens, n_blocks, leaves);
    return hipGetLastError();
}

hipError_t launch_merkle_nodes(const uint8_t* leaves, const uint8_t* log2w, uint32_t n, uint32_t log2_width,
                               uint8_t* roots, const uint8_t* expected, uint8_t* matched, hipStream_t stream) {
    return launch_nodes(n, log2_width, leaves, log2w, roots, expected, matched, stream);
}

hipError_t launch_merkle_leaf_check(const uint8_t* window, uint32_t row0, uint32_t n, uint32_t log2_width,
                                    uint32_t wpp, const uint32_t* leaf_first, const uint32_t* blocks,
                                    const uint8_t* expected_leaves, uint64_t* bad, uint8_t* shadow,
                                    uint8_t* leaves_out, hipStream_t stream) {
    if (n == 0 || (!expected_leaves && !leaves_out)) return hipSuccess;
    const uint64_t rows = (uint64_t)n << log2_width;
    const uint32_t grid = (uint32_t)((rows + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_leaf_check_kernel, dim3(grid), dim3(kBlock), 0, stream, window + (size_t)row0 * 32, n,
                       log2_width, wpp, leaf_first, blocks, expected_leaves,
                       reinterpret_cast<unsigned long long*>(bad), shadow ? shadow + (size_t)row0 * 32 : nullptr,
                       leaves_out);
    return hipGetLastError();
}

hipError_t launch_merkle_root(const uint8_t* layer, uint32_t n, uint8_t* work, uint8_t* root,
                              const uint8_t (*pads)[32], hipStream_t stream) {
    if (n == 1) return hipMemcpyAsync(root, layer, 32, hipMemcpyDeviceToDevice, stream);
    uint32_t total = 0;  // levels to the root: log2 of n rounded up to a power of two
    while ((1ull << total) < n) ++total;
    const uint8_t* in = layer;
    uint8_t* next = work;
    uint32_t m = n, done = 0;
    while (done < total) {
        const uint32_t levels = total - done < (uint32_t)kTileLog2 ? total - done : (uint32_t)kTileLog2;
        const uint32_t outs = (uint32_t)(((uint64_t)m + (1u << levels) - 1) >> levels);
        uint8_t* out = done + levels == total ? root : next;
        uint4 pad[2];  // rows are bytes: the words as the device loads them
        memcpy(pad, pads[done], 32);
        hipLaunchKernelGGL(merkle_layer_kernel, dim3(outs), dim3(kNodeBlock), 0, stream, in, m, levels, pad[0],
                           pad[1], out);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        in = out;
        next = out + (size_t)outs * 32;
        m = outs;
        done += levels;
    }
    return hipSuccess;
}

hipError_t launch_merkle_layers(const uint8_t* hashes, const struct vx_merkle_layers_plan& plan,
                                const vx_merkle_tile* tiles, uint8_t* work, uint8_t* roots, const uint8_t* expected,
                                uint8_t* matched, const uint8_t (*pads)[32], hipStream_t stream) {
    uint32_t first = 0;
    for (uint32_t p = 0; p < plan.passes; ++p) {
        uint4 pad[2];  // rows are bytes: the words as the device loads them
        memcpy(pad, pads[p], 32);
        hipLaunchKernelGGL(merkle_layers_kernel, dim3(plan.pass_tiles[p]), dim3(kNodeBlock), 0, stream,
                           p == 0 ? hashes : work, tiles + first, pad[0], pad[1], work, roots, expected, matched);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        first += plan.pass_tiles[p];
    }
    return hipSuccess;
}

hipError_t launch_merkle_trees(const uint8_t* hashes, const struct vx_merkle_tree_plan& plan,
                               const vx_merkle_tree_tile* tiles, uint8_t* tree, const uint8_t (*pads)[32],
                               hipStream_t stream) {
    uint32_t first = 0;
    for (uint32_t p = 0; p < plan.passes; ++p) {
        uint4 pad[2];  // rows are bytes: the words as the device loads them
        memcpy(pad, pads[p], 32);
        hipLaunchKernelGGL(merkle_tree_kernel, dim3(plan.pass_tiles[p]), dim3(kNodeBlock), 0, stream,
                           p == 0 ? hashes : tree, tiles + first, pad[0], pad[1], p == 0 ? 1u : 0u, tree);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        first += plan.pass_tiles[p];
    }
    return hipSuccess;
}

hipError_t launch_merkle_proofs(const uint8_t* hashes, const vx_merkle_proof* proofs, uint32_t n, uint8_t* tops,
                                const uint8_t* expected, uint8_t* matched, hipStream_t stream) {
    hipLaunchKernelGGL(merkle_proof_span_kernel, dim3(n), dim3(kNodeBlock), 0, stream, hashes, proofs, tops);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t grid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_proof_walk_kernel, dim3(grid), dim3(kBlock), 0, stream, hashes, proofs, n, tops,
                       expected, matched);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Leaf rows of unwritten blocks (the re-verify from disk over file holes,
// DESIGN.md §6.11): lane j writes SHA-256(lens[j] zero bytes), lens[j] in
// 1..16384, to leaf row rows[j] (NULL: row j).  Nothing is read but the two
// tables.  A full block's row is the same for every lane, so the caller passes
// it by value once it has it (have_full; made by this kernel with n = 1) and
// such a lane only stores; any other lane hashes from nothing: every schedule
// word of an all-zero block is zero, so a block is its 64 rounds with K[t]
// alone, run to the wave's largest block count under a select, and the last
// one or two blocks (zeros, 0x80, the bit length) take the general compression.
namespace {

constexpr sha256::ConstBlock zero_block() {  // K[t] + W[t] of an all-zero block: K[t]
    sha256::ConstBlock b{};
    for (int t = 0; t < 64; ++t) b.kw[t] = sha256::kK[t];
    return b;
}
__device__ constexpr sha256::ConstBlock kZeroBlock = zero_block();

__global__ __launch_bounds__(kBlock) void merkle_zero_leaf_kernel(const uint32_t* __restrict__ rows,
                                                                  const uint32_t* __restrict__ lens, uint32_t n,
                                                                  uint8_t* __restrict__ leaves, const uint4 full_lo,
                                                                  const uint4 full_hi, const uint32_t have_full) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t jj = j < n ? j : n - 1;  // lanes past n redo lane n-1 (in bounds) and store nothing
    const uint32_t len = lens[jj];
    const uint32_t row = rows ? rows[jj] : jj;
    const bool known = have_full && len == kLeaf;
    const uint32_t z = known ? 0u : len >> 6, rem = len & 63u;
    const uint32_t z_wave = __builtin_amdgcn_readfirstlane(wave_max(z));
    State s = sha256::iv();
    for (uint32_t b = 0; b < z_wave; ++b) {
        State t = s;
        sha256::compress_const(t, kZeroBlock);
        const bool mine = b < z;
#pragma unroll
        for (int k = 0; k < 8; ++k) s.h[k] = mine ? t.h[k] : s.h[k];
    }
    if (__builtin_amdgcn_readfirstlane(wave_max(known ? 0u : 1u))) {  // wave-uniform: some lane hashes
        uint32_t w[16];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) w[k] = k == (rem >> 2) ? 0x80000000u >> (8u * (rem & 3u)) : 0u;
        if (rem <= 55) w[15] = len << 3;  // a leaf is at most 16 KiB: the high word stays 0
        sha256::compress(s, w);
        if (rem > 55) {
#pragma unroll
            for (int k = 0; k < 15; ++k) w[k] = 0;
            w[15] = len << 3;
            sha256::compress(s, w);
        }
    }
    if (j >= n) return;
    if (known) {
        uint4* o = reinterpret_cast<uint4*>(leaves + (size_t)row * 32);
        o[0] = full_lo;
        o[1] = full_hi;
    } else {
        store_row(leaves, row, s);
    }
}

}  // namespace

hipError_t launch_merkle_zero_leaves(const uint32_t* rows, const uint32_t* lens, uint32_t n, uint8_t* leaves,
                                     const uint8_t* full_row, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    uint4 full[2] = {};  // rows are bytes: the words as the device stores them
    if (full_row) memcpy(full, full_row, 32);
    const uint32_t grid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(merkle_zero_leaf_kernel, dim3(grid), dim3(kBlock), 0, stream, rows, lens, n, leaves, full[0],
                       full[1], full_row ? 1u : 0u);
    return hipGetLastError();
}

}  // namespace vx
