// vx_kernels.h — internal launch interface between the C-ABI layer (the host
// units: vx_engine.hip, vx_slots.hip, vx_reverify.hip, vx_split.hip,
// vx_merkle.hip, vx_hybrid.hip) and the kernels (sha1_kernels.hip,
// sha1_tail_kernels.hip, sha256_kernels.hip, vx_gather.hip, vx_synth.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vx_hash.h"  // vx_merkle_tile, vx_merkle_layers_plan, vx_merkle_proof

namespace vx {

constexpr int kBlock = 256;  // 4 waves = one wave per SIMD of a CU
constexpr int kRing = 3;      // 128-byte groups in the ragged lane kernel's register ring
constexpr int kLaneRing = 4;  // ... and in the uniform lane kernel's (fenced, exact vmcnt)
constexpr int kPairBlock = 128;  // split kernel: consumer wave + producer wave

// Uniform-batch kernel variants (vx_tuning.h): 0 = default (best measured),
// 1 = lane-per-piece (one wave does everything), 2 = producer/consumer split.
// kSplitWide: the split kernel with one pair per CU (padded LDS), for
// batches bound by their longest chain with room to spare (plan_ragged).
enum UniformVariant {
    kUniformDefault = 0,
    kUniformLane = 1,
    kUniformSplit = 2,
    kSplitRing2 = 3,
    kSplitRing3 = 4,
    kSplitWide = 5
};
// LDS ring slots of the split kernels (sha1_kernels.hip "Ring protocol").
// 3: the producer runs two blocks ahead and the consumer prefetches the next
// block into registers while compressing (config 5 geometry 28.1 -> 26.6 ms,
// DESIGN.md §3.2).  2: the consumer reads each block at its top.  Variants
// 3 / 4 pin 2 / 3 slots for A/B runs.
constexpr int kSplitSlots = 3;
constexpr uint32_t kSplitMaxPieces = 16384;  // default picks split at or below this batch size

hipError_t launch_uniform(const uint8_t* base, uint64_t stride, uint32_t len, uint32_t n, uint8_t* digests,
                          const uint8_t* expected, uint8_t* matched, hipStream_t stream, int variant = 0,
                          const uint32_t* exp_index = nullptr);
hipError_t launch_uniform_lane(const uint8_t* base, uint64_t stride, uint32_t len, uint32_t n, uint8_t* digests,
                               const uint8_t* expected, uint8_t* matched, hipStream_t stream,
                               const uint32_t* exp_index = nullptr);
hipError_t launch_uniform_split(const uint8_t* base, uint64_t stride, uint32_t len, uint32_t n, uint8_t* digests,
                                const uint8_t* expected, uint8_t* matched, hipStream_t stream,
                                const uint32_t* exp_index = nullptr);

// Lane (kUniformLane), split (kUniformSplit) or split with one pair per CU
// (kSplitWide) for a ragged batch, from its longest piece and total bytes
// (DESIGN.md §3.4).
int plan_ragged(uint32_t n, uint64_t max_len, uint64_t total_len);

hipError_t launch_ragged(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens, const uint32_t* order,
                         uint32_t n, uint8_t* digests, const uint8_t* expected, uint8_t* matched,
                         hipStream_t stream, int variant = 0,
                          const uint32_t* exp_index = nullptr);
hipError_t launch_ragged_lane(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens,
                              const uint32_t* order, uint32_t n, uint8_t* digests, const uint8_t* expected,
                              uint8_t* matched, hipStream_t stream, const uint32_t* exp_index = nullptr);
hipError_t launch_ragged_split(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens,
                               const uint32_t* order, uint32_t n, uint8_t* digests, const uint8_t* expected,
                               uint8_t* matched, hipStream_t stream, const uint32_t* exp_index = nullptr);

// Resumable chunk kernel: lane j hashes bytes
// [poffs[j], poffs[j]+lens[j]) of piece pids[j] (total tlens[j]) from/to
// states[pid*5..]; the chunk that ends a piece emits digests/matched row pid
// (expected row pid).  Non-final chunk lengths must be multiples of 64.
hipError_t launch_chunk(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens, uint32_t n,
                        const uint32_t* pids, const uint64_t* poffs, const uint64_t* tlens, uint32_t* states,
                        uint8_t* digests, const uint8_t* expected, uint8_t* matched, hipStream_t stream);

// Zero-tail continuation of a hybrid torrent's padded v1 pieces
// (sha1_tail_kernels.hip).  Lane j finishes piece pid =
// pids[j] (NULL: j), lens[j] data bytes followed by pads[j] zero bytes,
// lens[j] + pads[j] == piece_length: from states[pid*5..] (the state after the
// lens[j] >> 6 whole data blocks; the IV when there are none, states is then
// not read) through the lens[j] & 63 tail bytes at base + tail_offs[j]
// (4-byte aligned), the zero blocks and the final padding block, to digests /
// matched row pid (expected row pid).  A lane with pads[j] == 0 stores nothing.
// TailSched: K(t) + W[t] of the final padding block of a total_len-byte
// message, total_len a multiple of 64 (expanded on the host by tail_sched).
struct TailSched {
    uint32_t kw[80];
};
void tail_sched(uint64_t total_len, TailSched* out);
hipError_t launch_zero_tail(const uint8_t* base, const uint64_t* tail_offs, const uint32_t* lens,
                            const uint32_t* pads, const uint32_t* pids, uint32_t n, uint64_t piece_length,
                            const uint32_t* states, uint8_t* digests, const uint8_t* expected, uint8_t* matched,
                            hipStream_t stream);
// A run of zeros inside a piece's chain (sha1_zero_run_kernel):
// lane j runs blocks[j] all-zero blocks from states[pids[j]*5..] (the IV when
// poffs[j] == 0, the row is then not read) and stores the state back to that
// row; no digest.  The pids of one launch are distinct.
hipError_t launch_zero_run(const uint32_t* pids, const uint32_t* poffs, const uint32_t* blocks, uint32_t n,
                           uint32_t* states, hipStream_t stream);
// vx_hybrid_device_pieces: launch_chunk's and launch_zero_tail's tables from
// device-resident offsets / lens / pads, and the two verdicts into one byte
// (bit 0 = v1, bit 1 = v2; either may be NULL).
hipError_t launch_hybrid_prep(const uint64_t* offsets, const uint32_t* lens, const uint32_t* pads, uint32_t n,
                              uint64_t* tail_offs, uint64_t* poffs, uint64_t* tlens, uint32_t* clens, uint32_t* pids,
                              hipStream_t stream);
hipError_t launch_hybrid_merge(const uint8_t* v1, const uint8_t* v2, uint32_t n, uint8_t* matched,
                               hipStream_t stream);
// SHA-1 of lens[j] zero bytes into digests row j, nothing read but lens
// (sha1_zero_kernel); digests 4-byte aligned.
hipError_t launch_sha1_zeros(const uint32_t* lens, uint32_t n, uint8_t* digests, hipStream_t stream);

// The end of a hybrid download slot (hybrid_finish_kernel):
// lane j finishes piece j when pads[j] != 0 (as launch_zero_tail with pids =
// NULL; every padded piece of the launch is padded_total bytes long, a
// multiple of 64) into digests row j, then compares digests row j and roots
// row j with row exp_index[j] (NULL: j) of exp_sha1 / exp_roots where
// flags[j] bit 0 / bit 1 is set, and writes the two verdict bits to
// matched[j].  A side whose flag bit is clear is not read.
hipError_t launch_hybrid_finish(const uint8_t* base, const uint64_t* tail_offs, const uint32_t* lens,
                                const uint32_t* pads, uint32_t n, uint64_t padded_total, const uint32_t* states,
                                uint8_t* digests, const uint8_t* roots, const uint8_t* exp_sha1,
                                const uint8_t* exp_roots, const uint32_t* exp_index, const uint8_t* flags,
                                uint8_t* matched, hipStream_t stream);

// Gather registered host pieces into a slot arena (vx_gather.hip, DESIGN.md
// §6.5): piece i (16-byte aligned device-mapped source src[i], length
// lens[i]) lands at arena + dst_off[i]; it owns 64 KiB tiles
// [tfirst[i], tfirst[i+1]) of the ntiles = tfirst[n] total.
uint32_t gather_tiles(uint32_t len);
hipError_t launch_gather(const uint64_t* src, const uint64_t* dst_off, const uint32_t* lens, const uint32_t* tfirst,
                         uint32_t n, uint32_t ntiles, uint8_t* arena, hipStream_t stream, uint32_t max_grid = 0);

// Zero-copy split kernel: piece i is read straight from
// registered host memory at its device-mapped address srcs[i] (16-byte
// aligned, lens[i] bytes; srcs[i] may be 0 when lens[i] == 0); digests /
// matched row i (expected row exp_index[i] when given).  loader: the
// three-wave form (a loader wave beside producer and consumer).
hipError_t launch_zero_copy(const uint64_t* srcs, const uint32_t* lens, uint32_t n, uint8_t* digests,
                            const uint8_t* expected, uint8_t* matched, bool loader, hipStream_t stream,
                            const uint32_t* exp_index = nullptr);

// BitTorrent v2 merkle kernels (sha256_kernels.hip): the leaf
// kernel writes all n << log2_width leaf rows, the node kernel reduces each
// piece's rows to its root (level log2w[i] when given) into roots and / or a
// verdict against expected.
constexpr int kMerkleMaxLog2Width = 17;
hipError_t launch_merkle_uniform(const uint8_t* base, uint64_t stride, uint32_t len, uint32_t last_len, uint32_t n,
                                 uint32_t log2_width, uint8_t* leaves, uint8_t* roots, const uint8_t* expected,
                                 uint8_t* matched, hipStream_t stream);
hipError_t launch_merkle_ragged(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens,
                                const uint8_t* log2w, uint32_t n, uint32_t log2_width, uint8_t* leaves,
                                uint8_t* roots, const uint8_t* expected, uint8_t* matched, hipStream_t stream);
// The fused piece kernel (the async path): as launch_merkle_ragged, but the
// leaf rows stay in LDS and are not kept.  log2_width <= 8: one launch, work
// unused.  Wider: work = tile tops ((n << (log2_width-8)) * 32 bytes) | log2w
// of the tops' trees (n bytes), both written by the piece kernel, then the
// node kernel over the tops.
inline uint64_t merkle_pieces_work(uint32_t n, uint32_t log2_width) {  // bytes of `work`
    return log2_width > 8 ? ((uint64_t)n << (log2_width - 8)) * 32 + n : 0;
}
hipError_t launch_merkle_pieces(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens,
                                const uint8_t* log2w, uint32_t n, uint32_t log2_width, uint8_t* work, uint8_t* roots,
                                const uint8_t* expected, uint8_t* matched, hipStream_t stream);
// The zero-copy piece kernel (vx_set_merkle_zero_copy): as
// launch_merkle_pieces, but piece i is read at the device-visible address
// srcs[i] (HBM, or a registered host buffer's mapping; 16-byte aligned; may be
// 0 when lens[i] == 0) with cooperative loads.  work as merkle_pieces_work says.
// merkle_zc_geometry: leaves per workgroup, leaves per wave, bytes per leaf
// per tile, tiles in flight per wave (host-only).
hipError_t launch_merkle_zc_pieces(const uint64_t* srcs, const uint32_t* lens, const uint8_t* log2w, uint32_t n,
                                   uint32_t log2_width, uint8_t* work, uint8_t* roots, const uint8_t* expected,
                                   uint8_t* matched, hipStream_t stream);
void merkle_zc_geometry(uint32_t out[4]);
// The block check (vx_merkle_device_block_check): the ragged batch's leaves
// against row g of expected_leaves, one bit per block into bad (uint64 words,
// max(1, 2^log2_width / 64) per piece, every word written) and / or the leaf
// rows into leaves_out.  expected_leaves and bad are both given or both NULL;
// n >= 1.
hipError_t launch_merkle_block_check(const uint8_t* base, const uint64_t* offsets, const uint32_t* lens, uint32_t n,
                                     uint32_t log2_width, const uint8_t* expected_leaves, uint64_t* bad,
                                     uint8_t* leaves_out, hipStream_t stream);
// The two halves on their own (the re-verify from disk): the block kernel
// hashes stage block b (lens[b] <= 16384 bytes at stage + b*16384) into leaf
// row rows[b] (0xFFFFFFFF: none; lens[b] == 0: the zero hash, nothing read);
// the node kernels reduce n pieces' rows that are already in leaves.
hipError_t launch_merkle_blocks(const uint8_t* stage, const uint32_t* rows, const uint32_t* lens, uint32_t n_blocks,
                                uint8_t* leaves, hipStream_t stream);
hipError_t launch_merkle_nodes(const uint8_t* leaves, const uint8_t* log2w, uint32_t n, uint32_t log2_width,
                               uint8_t* roots, const uint8_t* expected, uint8_t* matched, hipStream_t stream);
// The leaf check (merkle_leaf_check_kernel, DESIGN.md §3.7 "Block checks from
// disk"): the n pieces of one vx_merkle::Nodes entry, piece k's 2^log2_width
// rows at row row0 + (k << log2_width) of window; blocks[k] of them are live
// and belong at row leaf_first[k] on of the compact leaf table.  With
// expected_leaves (and bad; shadow may be NULL): the live rows against that
// table, piece k's bits into words bad[k * wpp ..] (wpp >= max(1,
// 2^log2_width / 64); words the group does not cover are left alone), and the
// stored rows, zeros at dead slots, into shadow at the window's rows.  With
// leaves_out: the live rows into that table.  Neither: nothing is launched.
hipError_t launch_merkle_leaf_check(const uint8_t* window, uint32_t row0, uint32_t n, uint32_t log2_width,
                                    uint32_t wpp, const uint32_t* leaf_first, const uint32_t* blocks,
                                    const uint8_t* expected_leaves, uint64_t* bad, uint8_t* shadow,
                                    uint8_t* leaves_out, hipStream_t stream);
// Leaf rows of unwritten blocks (merkle_zero_leaf_kernel):
// SHA-256 of lens[j] (1..16384) zero bytes into leaf row rows[j] (NULL: j),
// nothing read but the tables.  full_row (host, 32 bytes, may be NULL): the row
// of a full 16 KiB block, stored as is where lens[j] == 16384.
hipError_t launch_merkle_zero_leaves(const uint32_t* rows, const uint32_t* lens, uint32_t n, uint8_t* leaves,
                                     const uint8_t* full_row, hipStream_t stream);
// Root of a layer of n >= 1 hashes; pads[k] = the pad hash of the layer's
// height + k (one per level to the root); work: 32*n bytes.
hipError_t launch_merkle_root(const uint8_t* layer, uint32_t n, uint8_t* work, uint8_t* root,
                              const uint8_t (*pads)[32], hipStream_t stream);
// Many layers in plan.passes launches (vx_merkle_device_layers): tiles is the
// device copy of the planner's tiles, pads[p] the pad hash of the layers'
// height + 9p, work plan.work_rows rows.
hipError_t launch_merkle_layers(const uint8_t* hashes, const struct vx_merkle_layers_plan& plan,
                                const vx_merkle_tile* tiles, uint8_t* work, uint8_t* roots, const uint8_t* expected,
                                uint8_t* matched, const uint8_t (*pads)[32], hipStream_t stream);
// The trees of many layers in plan.passes launches (vx_merkle_device_trees):
// tiles is the device copy of the planner's tiles, pads[p] the pad hash of the
// layers' height + 9p, tree plan.tree_rows rows.
hipError_t launch_merkle_trees(const uint8_t* hashes, const struct vx_merkle_tree_plan& plan,
                               const vx_merkle_tree_tile* tiles, uint8_t* tree, const uint8_t (*pads)[32],
                               hipStream_t stream);
// Hash proofs in two launches (vx_merkle_device_proofs): the spans' roots into
// tops, then the uncle walks, the tops in place and the verdicts.
hipError_t launch_merkle_proofs(const uint8_t* hashes, const vx_merkle_proof* proofs, uint32_t n, uint8_t* tops,
                                const uint8_t* expected, uint8_t* matched, hipStream_t stream);

hipError_t launch_synth_fill(uint8_t* base, uint64_t stride, uint32_t len, uint32_t n, uint64_t first,
                             uint64_t seed, uint32_t corrupt_every, hipStream_t stream);

}  // namespace vx
