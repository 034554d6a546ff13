/*
 * vx_tuning.h — measurement and test entry points, NOT part of the drop-in
 * boundary.  They are exported only by the test/tuning build
 * libvortex_amd_tuning.so (the same sources, linked with -DVX_TEST_HOOKS);
 * the library vortex links, libvortex_amd.so, exports vx_hash.h alone
 * (tests/test_abi.py checks both export lists with nm -D).  Unstable: these
 * may change in any release without an ABI version bump.
 *
 * Kernel variants (vx_sha1_device_*_variant): 0 = default (what
 * vx_sha1_device_uniform / _ragged run), 1 = lane-per-piece (one wave per 64
 * pieces does loads, schedule and rounds), 2 = producer/consumer split (a
 * load+schedule wave feeds a rounds-only wave through an LDS ring), 3 / 4 =
 * split with a 2- / 3-slot LDS ring (A/B of the ring protocol; 2 uses the
 * default ring), 5 = split with one pair per CU (ragged only; what the
 * planner picks for batches bound by their longest chain).
 */
#ifndef VX_TUNING_H
#define VX_TUNING_H
#include <stddef.h>
#include <stdint.h>
/* Compile-time A/B of the v2 async path's kernel (vx_merkle_submit, DESIGN.md
 * §3.7): 1 (the default) hashes a v2 slot with the fused piece kernel, leaves
 * reduced in LDS; 0 with the leaf + node kernels of vx_merkle_device_ragged
 * and a leaf array per slot.  Build the engine with -DVX_MERKLE_ASYNC_FUSED=0
 * for the other leg. */
#ifndef VX_MERKLE_ASYNC_FUSED
#define VX_MERKLE_ASYNC_FUSED 1
#endif

#ifdef __cplusplus
extern "C" {
#endif

int vx_sha1_device_ragged_variant(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                                  const uint32_t* d_order, uint32_t n, void* d_digests, const void* d_expected,
                                  void* d_matched, void* stream, int variant);
struct vx_ctx;
struct vx_split;
/* How a context with zero_copy = 1 hashes a slot of n registered, aligned
 * pieces of total_len bytes: 1 the zero-copy pair, 2 the zero-copy kernel
 * with a loader wave (n < 128, a latency-bound batch); 0 (gather + hash) is
 * only taken with zero_copy = 0.  Host-only. */
int vx_tuning_zero_copy_plan(uint32_t n, uint64_t total_len);
/* The zero-copy kernel on its own (A/B probes): piece i is d_lens[i] bytes at
 * the device-visible address d_srcs[i] (HBM, or a registered host buffer's
 * device mapping), 16-byte aligned; d_digests n x 20 B, d_expected /
 * d_matched optional.  loader = 0: the pair form, 1: the three-wave form.
 * Enqueue-only on `stream` (a hipStream_t or NULL). */
int vx_tuning_zero_copy_kernel(const uint64_t* d_srcs, const uint32_t* d_lens, uint32_t n, void* d_digests,
                               const void* d_expected, void* d_matched, int loader, void* stream);
/* The zero-tail kernel on its own (tools/hybrid_tail_bench.py):
 * lane j finishes a piece of d_lens[j] data bytes followed by d_pads[j] zeros,
 * d_lens[j] + d_pads[j] == piece_length (a multiple of 64), from
 * d_states[5j..] (the state after its d_lens[j] >> 6 whole data blocks)
 * through the d_lens[j] & 63 tail bytes at d_base + d_tail_offs[j]; d_digests
 * n x 20 B.  Enqueue-only on `stream`. */
int vx_tuning_zero_tail_kernel(const void* d_base, const uint64_t* d_tail_offs, const uint32_t* d_lens,
                               const uint32_t* d_pads, uint32_t n, uint64_t piece_length, const uint32_t* d_states,
                               void* d_digests, void* stream);
/* The chunked SHA-1 kernel on its own (the same tool): lane j
 * hashes d_lens[j] bytes at d_base + d_offsets[j] (16-byte aligned) as bytes
 * [d_poffs[j], +d_lens[j]) of piece d_pids[j], d_tlens[j] bytes in all, from /
 * to d_states[5 * pid..]; a chunk that ends its piece writes d_digests row
 * pid, any other (a multiple of 64 bytes) stores the state.  Enqueue-only. */
int vx_tuning_chunk_kernel(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t n,
                           const uint32_t* d_pids, const uint64_t* d_poffs, const uint64_t* d_tlens,
                           uint32_t* d_states, void* d_digests, void* stream);
/* The zero-run kernel on its own (DESIGN.md §3.8, §6.11;
 * tests/test_gpu_hybrid_zero_run.py): lane j runs d_blocks[j] all-zero 64-byte
 * blocks from d_states[5 * d_pids[j]..] (from the initial value when
 * d_poffs[j] == 0: the row is then not read) and stores the state back to that
 * row.  The d_pids of a launch are distinct.  Enqueue-only on `stream`. */
int vx_tuning_zero_run_kernel(const uint32_t* d_pids, const uint32_t* d_poffs, const uint32_t* d_blocks, uint32_t n,
                              uint32_t* d_states, void* stream);
/* merkle_zero_leaf_kernel on its own: leaf row d_rows[j] (NULL: row j) of d_leaves =
 * SHA-256 of d_lens[j] zero bytes, d_lens[j] in 1..16384; full_row (HOST, 32 bytes, may be
 * NULL): stored as is where d_lens[j] == 16384.  The d_rows of a launch are distinct.
 * Enqueue-only on `stream`. */
int vx_tuning_zero_leaf_kernel(const uint32_t* d_rows, const uint32_t* d_lens, uint32_t n,
                               void* d_leaves, const void* full_row, void* stream);
/* merkle_zc_piece_kernel on its own (vx_set_merkle_zero_copy, DESIGN.md §3.7;
 * tests/test_gpu_merkle_zc_sweep.py): the launch and, above 256 leaves, the
 * node pass over the tile tops, and nothing else.  Piece i is d_lens[i] bytes
 * at the device-visible address d_srcs[i] (HBM, or a registered host buffer's
 * device mapping; 16-byte aligned; not read when d_lens[i] == 0), its tree has
 * 2^d_log2w[i] leaf slots (NULL: 2^log2_width), d_lens[i] <= 16384 <<
 * d_log2w[i] and d_log2w[i] <= log2_width; d_roots n x 32 B and / or d_expected
 * with d_matched, as vx_merkle_device_pieces takes them.  The tile tops are the
 * call's own (one process-wide block, grown on demand: calls on different
 * streams must not overlap above log2_width 8).  Enqueue-only on `stream`. */
int vx_tuning_merkle_zc_kernel(const uint64_t* d_srcs, const uint32_t* d_lens, const uint8_t* d_log2w, uint32_t n,
                               uint32_t log2_width, void* d_roots, const void* d_expected, void* d_matched,
                               void* stream);
/* That kernel's geometry (host-only): out[0] leaf rows per workgroup, out[1]
 * leaves a wave loads and hashes, out[2] bytes per leaf per cooperative tile,
 * out[3] tiles in flight per wave.  LDS per workgroup: out[0] / out[1] stages
 * of out[2] / 16 rows of out[1] + 1 16-byte slots, and out[0] 32-byte rows. */
void vx_tuning_merkle_zc_geometry(uint32_t* out); /* out[4] */
/* gather_kernel on its own (tests/test_gpu_gather_sweep.py):
 * vx::launch_gather and nothing else.  Piece i is d_lens[i] bytes at the
 * device-visible address d_src[i] and goes to d_arena + d_dst_off[i]; a piece
 * the launch does not gather (d_src[i] == 0) or of no bytes owns no tile and
 * is not touched.  The caller's contract, as the engine keeps it: d_arena,
 * every gathered d_src[i] and every d_dst_off[i] are 16-byte aligned, piece i
 * owns the 64 KiB tiles [d_tfirst[i], d_tfirst[i + 1]) (d_tfirst has n + 1
 * entries, d_tfirst[i + 1] - d_tfirst[i] == ceil(d_lens[i] / 64 KiB) for a
 * gathered piece and 0 otherwise), and ntiles == d_tfirst[n].  max_grid caps
 * the workgroups of the launch, 0: the default of 64.  n == 0 or ntiles == 0
 * launches nothing.  Enqueue-only on `stream`. */
int vx_tuning_gather_kernel(const uint64_t* d_src, const uint64_t* d_dst_off, const uint32_t* d_lens,
                            const uint32_t* d_tfirst, uint32_t n, uint32_t ntiles, void* d_arena, uint32_t max_grid,
                            void* stream);
/* The kernel that ends a hybrid download slot on its own (DESIGN.md §3.8,
 * §6.9; tests/test_gpu_hybrid_tail_sweep.py): lane j with d_pads[j] != 0
 * finishes its piece as the zero-tail kernel does (every padded piece is
 * padded_total bytes, a multiple of 64) into d_digests row j; every lane then
 * compares d_digests row j and d_roots row j (n x 32 B) with row
 * d_exp_index[j] (NULL: j) of d_exp_sha1 / d_exp_roots where d_flags[j] bit 0 /
 * bit 1 is set, and writes the verdict bits to d_matched[j].  Enqueue-only. */
int vx_tuning_hybrid_finish_kernel(const void* d_base, const uint64_t* d_tail_offs, const uint32_t* d_lens,
                                   const uint32_t* d_pads, uint32_t n, uint64_t padded_total,
                                   const uint32_t* d_states, void* d_digests, const void* d_roots,
                                   const void* d_exp_sha1, const void* d_exp_roots, const uint32_t* d_exp_index,
                                   const uint8_t* d_flags, void* d_matched, void* stream);
/* Fault injection for tests: after k more successful piece submits (async or
 * inside a host batch), the next one fails with VX_ENOMEM without latching
 * the context, as a failed pinned-stage allocation does.  k < 0 turns it off. */
void vx_tuning_fail_submit_after(struct vx_ctx* ctx, int64_t k);
/* Fault injection for tests: after k more successful batch launches, the next
 * launch fails as a device error does (VX_EDEVICE, the context turns sticky):
 * the recovery path of INTEGRATION.md "Device failure".  k < 0 turns it off. */
void vx_tuning_fail_launch_after(struct vx_ctx* ctx, int64_t k);
/* A/B of the file re-verify's copy placement: mode 1 (the
 * default) puts every chunk round's data H2D on the context's one
 * high-priority copy stream and its lane table on the slot's stream; 0 puts
 * both on the slot's stream behind a host wait for the previous round's copy
 * (round 4's form). */
void vx_tuning_verify_copy_stream(struct vx_ctx* ctx, int mode);
/* A/B of the pinned stages' memory: on = 1 allocates them as
 * 2 MiB-aligned transparent-huge-page mappings registered with hipHostRegister,
 * 0 with hipHostMalloc.  Idle stages are freed and reallocated on next use. */
void vx_tuning_stage_huge(struct vx_ctx* ctx, int on);
/* What the engine holds of the runtime in this process, over every context:
 * four counts: out[0] device blocks, out[1] pinned blocks (stages included), out[2] streams,
 * out[3] events.  Everything the engine owns is counted where it is made and
 * where it is given back, so a context that is destroyed leaves the counts as
 * they were before it was created. */
void vx_tuning_live_resources(uint64_t* out);
/* Fault injection for tests, process-wide as the counts are: after n more
 * successful creations of a block, stream or event, the next one fails on the
 * host before the runtime is asked (the call returns VX_ENOMEM or VX_EDEVICE as
 * it does when the runtime refuses), and the hook turns itself off.  n < 0
 * turns it off. */
void vx_tuning_fail_alloc_after(int64_t n);
/* A/B of the split's rules for pieces of one chunk (vx_verify_files_split,
 * DESIGN.md §6.6): one_round = 1 (the default) lets their groups keep the
 * first group's rule until the rates are in, skips the tenth rule and reads
 * runs of them with one pread, 2 does the same piece by piece, 0 gives them
 * the multi-round pieces' rules; round_cap > 0 (default 64 MiB) caps
 * their rounds at that many bytes but no fewer than 1,024 lanes, 0 gives them
 * the slot's whole stage.  lag = 1 (the default) adds the learned lag to the
 * first group's T_engine, 0 keeps learning it without adding it.  learn = 1
 * (the default) starts each call from the median of the last five calls'
 * figures, 0 from their running mean (each call weighted 1/2). */
void vx_tuning_split_rules(struct vx_ctx* ctx, int one_round, uint64_t round_cap, int lag, int learn);
/* The kernel vx_sha1_device_ragged_hint runs for a batch of n pieces whose
 * longest is max_len bytes, total_len bytes in all: 1 = lane, 2 = split,
 * 5 = split with one pair per CU (host-only). */
int vx_tuning_plan_ragged(uint32_t n, uint32_t max_len, uint64_t total_len);
/* The file re-verify's round boundaries for a window whose longest piece is
 * L bytes with chunk C (head/tail: ramp the first / last C bytes down to
 * C/4).  Writes up to max (offset, length) pairs to out
 * (2*max uint64_t) and returns the number of rounds (host-only). */
size_t vx_tuning_chunk_schedule(uint64_t L, uint64_t C, int head, int tail, uint64_t* out, size_t max);
/* The engine's side of the split's claim word (vx_verify_files_split):
 * take up to k pieces from the top of the unclaimed range; returns the new
 * stop and (was, may be NULL) the stop before, so the pieces taken are
 * [returned, *was) (host-only). */
uint64_t vx_tuning_split_take_tail(struct vx_split* s, uint64_t k, uint64_t* was);
/* The last vx_verify_files_split call's decisions, one row of 13 doubles per
 * round it formed: ms since the call's start, the pool's rate (pieces/s), the
 * engine's intake rate (B/s), its chain per 64-byte block (ns), the predicted
 * remaining ms of the engine and of the pool with the group taken, unclaimed
 * pieces, the group taken, active lanes, the pool's finished pieces, the
 * decision mode (0 later round, 1 first, 2 forced), whether both sides'
 * rates were measured, and the learned lag (ms) inside the engine's time.
 * Writes up to max rows; returns the row count. */
size_t vx_tuning_last_split(const struct vx_ctx* ctx, double* out, size_t max);

int vx_sha1_device_uniform_variant(const void* d_base, uint64_t stride, uint32_t len, uint32_t n, void* d_digests,
                                   const void* d_expected, void* d_matched, void* stream, int variant);

/* Shader-clock stamps (bench.py; vx_clock.hip): enqueue `blocks` one-wave
 * workgroups on `stream`; workgroup b writes d_out[3b..3b+2] = (shader cycle
 * counter, 100 MHz real-time counter, XCC id).  Two stamps bracketing a
 * stretch of work on one stream give each XCC's mean shader clock over it. */
int vx_tuning_clock_stamp(void* d_out, uint32_t blocks, void* stream);
/* The real-time counter's rate in kHz (hipDeviceAttributeWallClockRate). */
int vx_tuning_wall_clock_khz(int device);
/* Physical identity of HIP device `device`: its PCI bus id ("dddd:bb:dd.f",
 * NUL-terminated in bus_id[0..len), len >= 16) and 16-byte UUID. */
int vx_tuning_device_identity(int device, char* bus_id, size_t len, char* uuid16);

#ifdef __cplusplus
}
#endif
#endif
