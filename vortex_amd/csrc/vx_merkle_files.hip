// vx_merkle_files.hip — the BitTorrent v2 files calls of vx_hash.h:
// vx_merkle_verify_files / _range (the re-verify from disk),
// vx_merkle_hash_files / _range and their forms that check or keep the 16 KiB
// leaf layer (_verify_files_blocks, _hash_files_leaves, with _leaf_rows and
// _device_leaf_check), with the buffers they keep in the context and
// file_trees, which the hybrid hash call shares.  Every other v2 entry is in
// vx_merkle.hip.
//
// Rounds of 16 KiB blocks packed by vx_merkle::Rounds, one slot's pinned stage
// each, run by vx_block_rounds.hpp.  Per round, on the slot's stream: the data
// H2D, the rows | lens table in one H2D, the block kernel, and the node kernels
// of the groups of pieces the round finished, with verdicts into the call's
// device rows; the kernels wait for the previous round's (one event), the copies
// do not.  A call with a leaf table adds, per finished group, the leaf-check
// kernel and (checking) a second node launch over the shadow window.
#include "vx_engine_internal.hpp"
#include "vx_merkle_leaves.hpp"

using namespace vxe;

int vxe::file_trees(vx_ctx* c, const uint8_t* d_rows, const uint64_t* file_lengths, size_t nfiles,
                    uint32_t piece_length, const std::vector<uint8_t>& bad, uint8_t* tree_out, hipStream_t st,
                    const std::string& who) {
    if (int rc = set_device(c)) return rc;
    std::vector<uint32_t> counts;  // of the non-empty files: their pieces are d_rows, back to back
    for (size_t f = 0; f < nfiles; ++f)
        if (file_lengths[f]) counts.push_back((uint32_t)((file_lengths[f] + piece_length - 1) / piece_length));
    if (counts.empty()) return 0;
    struct vx_merkle_tree_plan plan;
    if (vx_merkle::plan_trees(counts.data(), (uint32_t)counts.size(), &plan, nullptr, 0, nullptr))
        return fail(VX_EINVAL, who + ": the files' trees hold 2^32 rows or more");
    std::vector<vx_merkle_tree_tile> tiles(plan.n_tiles);
    std::vector<uint64_t> off(counts.size() + 1);
    (void)vx_merkle::plan_trees(counts.data(), (uint32_t)counts.size(), &plan, tiles.data(), tiles.size(), off.data());
    uint32_t height = 0;
    while (((uint32_t)VX_MERKLE_BLOCK << height) < piece_length) ++height;
    DeviceMem block;  // (the call waits for st before it returns, error or not)
    if (!block.reserve(plan.tree_rows * 32 + tiles.size() * sizeof(vx_merkle_tree_tile)))
        return fail(VX_ENOMEM, who + ": tree buffer allocation failed");
    uint8_t* const d = block.get();
    uint8_t* d_tiles = d + plan.tree_rows * 32;
    int rc = 0;
    if (hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(vx_merkle_tree_tile), hipMemcpyHostToDevice, st) !=
        hipSuccess)
        rc = fail(VX_EDEVICE, who + ": tile upload failed");
    if (!rc)
        rc = vx_merkle_device_trees(d_rows, &plan, reinterpret_cast<const vx_merkle_tree_tile*>(d_tiles), height, d, st);
    if (!rc && hipMemcpyAsync(tree_out, d, plan.tree_rows * 32, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(VX_EDEVICE, who + ": tree download failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail(VX_EDEVICE, who + ": the tree passes failed");
    if (rc) return rc;
    uint64_t piece = 0;
    for (size_t k = 0; k < counts.size(); ++k) {  // never a tree over bytes that were not read
        bool any = false;
        for (uint32_t j = 0; j < counts[k]; ++j) any |= bad[piece + j] != 0;
        if (any) std::memset(tree_out + off[k] * 32, 0, (off[k + 1] - off[k]) * 32);
        piece += counts[k];
    }
    return 0;
}

constexpr uint64_t kMerkleRoundCap = 64ull << 20;  // a round's stage bytes at most
constexpr uint32_t kMerkleRunBlocks = 128;         // one pread: 2 MiB at most (32 reads for 16 readers per full round)

// What vx_merkle_verify_files keeps in the context, grown on demand (a block that
// grows is allocated anew: nothing in it outlives a call).
static int ensure_merkle_files(vx_ctx* c, uint64_t window_rows, uint64_t entries, uint64_t count) {
    vx_ctx::MerkleFiles& m = c->mfiles;
    const char* oom = "vx_merkle_verify_files: buffer allocation failed";
    if (!m.chain && !m.chain.make(hipEventDisableTiming))
        return fail(VX_EDEVICE, "vx_merkle_verify_files: event creation failed");
    if (m.window_rows < window_rows) {
        m.window_rows = m.d_window.reserve(window_rows * 32) ? window_rows : 0;
        if (!m.window_rows) return fail(VX_ENOMEM, oom);
    }
    if (m.tab_entries < entries || m.h_tab.size() != c->slots.size()) {
        m.tab_entries = 0;
        m.h_tab.resize(c->slots.size());
        m.d_tab.resize(c->slots.size());
        for (size_t k = 0; k < c->slots.size(); ++k)
            if (!m.h_tab[k].reserve(entries * 8) || !m.d_tab[k].reserve(entries * 8)) return fail(VX_ENOMEM, oom);
        m.tab_entries = entries;
    }
    if (m.call_cap < count) {
        const uint64_t cap = std::max<uint64_t>(count, 4096);
        m.call_cap = m.d_call.reserve(cap * 34) ? cap : 0;
        if (!m.call_cap) return fail(VX_ENOMEM, oom);
    }
    return 0;
}

// What the calls with a leaf table add to merkle_files_impl.  Checking
// (vx_merkle_verify_files_blocks): expected_leaves, bad_out and the optional
// layer_ok_out / bad_counts_out.  Keeping (vx_merkle_hash_files_leaves):
// leaves_out.  Both tables are the whole torrent's, leaf_rows rows.
struct LeafTable {
    const uint8_t* expected_leaves = nullptr;
    uint8_t* leaves_out = nullptr;
    uint64_t leaf_rows = 0;
    uint8_t* layer_ok_out = nullptr;
    uint64_t* bad_out = nullptr;
    uint32_t* bad_counts_out = nullptr;
};

// The leaf row of a full unwritten block, made once per
// context by the zero-leaf kernel itself with n = 1 (there is no host SHA-256)
// and passed to every later launch by value (the hybrid files call shares it).
int vxe::zero_leaf_row(vx_ctx* c, const char* who) {
    vx_ctx::Holes& h = c->holes;
    if (h.have_zero_leaf) return 0;
    int rc = ensure_holes(c, who);
    if (rc) return rc;
    const uint32_t len = VX_MERKLE_BLOCK;
    uint8_t *const hh = h.h.get(), *const hd = h.d.get();
    std::memcpy(hh, &len, sizeof(len));
    hipError_t e = hipMemcpyAsync(hd, hh, sizeof(len), hipMemcpyHostToDevice, h.stream);
    if (e == hipSuccess) e = hipEventRecord(h.t0, h.stream);
    if (e == hipSuccess)
        e = vx::launch_merkle_zero_leaves(nullptr, h.d.as<const uint32_t>(), 1, hd + h.kLeafAt, nullptr,
                                          h.stream);
    if (e == hipSuccess) e = hipEventRecord(h.t1, h.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hh + h.kLeafAt, hd + h.kLeafAt, 32, hipMemcpyDeviceToHost, h.stream);
    const hipError_t sync = hipStreamSynchronize(h.stream);
    if (e != hipSuccess || sync != hipSuccess)
        return hip_fail(e != hipSuccess ? e : sync, (std::string(who) + ": zero leaf row").c_str());
    float ms = 0;
    if (hipEventElapsedTime(&ms, h.t0, h.t1) == hipSuccess) h.last.zero_hash_ms += ms;
    std::memcpy(h.zero_leaf, hh + h.kLeafAt, 32);
    h.have_zero_leaf = true;
    return 0;
}

// rows_out set: the hash call (vx_merkle_hash_files).  No expected table; the
// node kernels write the pieces' rows where the verify call keeps the expected
// ones, matched_out is the call's ok_out (may be NULL), and with tree_out the
// files' trees are built from those rows after the last round.
static int64_t merkle_files_impl(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                                 uint32_t piece_length, const uint8_t* expected, size_t n_pieces, size_t first,
                                 size_t count, uint8_t* matched_out, uint32_t io_threads, uint8_t* rows_out = nullptr,
                                 uint8_t* tree_out = nullptr, uint64_t tree_rows = 0,
                                 const LeafTable* lt = nullptr) {
    const bool hashing = rows_out != nullptr;
    const bool checking = lt && !hashing;  // block by block, against lt->expected_leaves
    const std::string who = hashing ? (lt ? "vx_merkle_hash_files_leaves" : "vx_merkle_hash_files")
                                    : (lt ? "vx_merkle_verify_files_blocks" : "vx_merkle_verify_files");
    const bool null_args = (nfiles && (!paths || !file_lengths)) ||
                           (!hashing && ((n_pieces && !expected) || (count && !matched_out))) ||
                           (lt && lt->leaf_rows && !(hashing ? (const void*)lt->leaves_out : lt->expected_leaves)) ||
                           (checking && count && !lt->bad_out);
    int rc = begin_block_call(c, who, null_args, "paths/file_lengths/expected/matched_out/leaf table/bad_out",
                              file_lengths, nfiles, piece_length, n_pieces, first, count, UINT64_MAX, tree_out,
                              tree_rows);
    if (rc) return rc;
    if (lt && lt->leaf_rows != vx_merkle::torrent_leaf_rows(file_lengths, nfiles))
        return fail(VX_EINVAL, who + ": leaf_rows is not what vx_merkle_leaf_rows returns");
    if (count == 0) return 0;
    vx_merkle::LeafRange lr;
    if (lt && !vx_merkle::leaf_range(file_lengths, nfiles, piece_length, first, count, lr))
        return fail(VX_ERANGE, who + ": the range holds 2^32 leaf rows or more");
    const uint32_t wpp = std::max<uint32_t>(1, piece_length / VX_MERKLE_BLOCK / 64);  // bitmap words per piece
    const uint64_t bpr64 = std::min<uint64_t>(c->slots[0].arena_cap, kMerkleRoundCap) / VX_MERKLE_BLOCK;
    if (bpr64 == 0) return fail(VX_ERANGE, who + ": a slot holds no 16 KiB block");
    const uint32_t bpr = (uint32_t)bpr64;
    if ((rc = set_device(c))) return rc;
    const uint32_t R = vx_merkle::Rounds::window_for(bpr, piece_length);
    const uint32_t entries = 2 * bpr + piece_length / VX_MERKLE_BLOCK;
    if ((rc = ensure_merkle_files(c, R, entries, count))) return rc;
    vx_ctx::MerkleFiles& mf = c->mfiles;
    uint8_t *d_exp = mf.d_call.get(), *d_match = d_exp + mf.call_cap * 32, *d_lw = d_exp + mf.call_cap * 33;
    // The leaf table's part: the range's rows (uploaded here as d_exp is, or
    // downloaded after the last round), leaf_first | blocks | layer_ok per
    // piece, and when checking the shadow window and the bitmap, cleared once:
    // a group narrower than the call writes only the words it covers.
    const uint64_t words = (uint64_t)count * wpp;
    if (lt && mf.piece_cap < count) {
        const uint64_t cap = std::max<uint64_t>(count, 4096);
        mf.piece_cap = mf.d_piece.reserve(cap * 9) ? cap : 0;
    }
    if ((lt && (!mf.piece_cap || !mf.d_leaf.reserve(lr.rows * 32))) ||
        (checking && (!mf.d_shadow.reserve(mf.window_rows * 32) || !mf.d_bad.reserve(words * 8))))
        return fail(VX_ENOMEM, who + ": leaf-table buffer allocation failed");
    uint8_t *const d_window = mf.d_window.get(), *const d_leaf = mf.d_leaf.get(), *const d_shadow = mf.d_shadow.get();
    uint64_t* const d_bad = mf.d_bad.as<uint64_t>();
    uint32_t* d_first = mf.d_piece.as<uint32_t>();
    uint32_t* d_blocks = d_first + mf.piece_cap;
    uint8_t* d_layer_ok = mf.d_piece.get() + mf.piece_cap * 8;

    BlockCall call{c, who, first, count};
    bool up = hashing || hipMemcpy(d_exp, expected + 32 * first, count * 32, hipMemcpyHostToDevice) == hipSuccess;
    if (lt)
        up = up && hipMemcpy(d_first, lr.leaf_first.data(), count * 4, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(d_blocks, lr.blocks.data(), count * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (checking)  // (call.begin waits for the null stream)
        up = up && hipMemcpy(d_leaf, lt->expected_leaves + lr.base * 32, lr.rows * 32, hipMemcpyHostToDevice) ==
                       hipSuccess &&
             hipMemsetAsync(d_bad, 0, words * 8, nullptr) == hipSuccess &&
             hipMemsetAsync(d_layer_ok, 0, count, nullptr) == hipSuccess;
    if ((rc = call.begin(up, paths, file_lengths, nfiles, piece_length, d_lw, d_match, count, matched_out))) return rc;
    // Blocks that lie wholly in file holes are not read: the
    // packer leaves them out of the stage and a kernel of their own writes
    // their leaf rows.  The hash call does not ask.
    c->holes.last = vx_hole_trace{};
    const vx_extents::Holes holes = hashing ? vx_extents::Holes() : scan_holes(c, call.fds, file_lengths);
    vx_merkle::HolePredicate in_hole;
    if (holes.any()) {
        in_hole = [&holes](uint32_t f, uint64_t off, uint32_t len) { return holes.hole(f, (int64_t)off, len); };
        if ((rc = zero_leaf_row(c, who.c_str()))) return call.end(rc, 0);
    }
    // One round on slot si's stream, its data already in the stage.
    auto enqueue = [&](size_t si, const vx_merkle::Round& r) -> int {
        Slot& s = c->slots[si];
        // the tables: rows | lens, each the block kernel's m entries, then the hole blocks'
        const uint32_t all = (uint32_t)r.rows.size(), m = all - r.hole_blocks;
        uint32_t *h_tab = mf.h_tab[si].as<uint32_t>(), *d_tab = mf.d_tab[si].as<uint32_t>();
        std::memcpy(h_tab, r.rows.data(), (size_t)all * 4);
        std::memcpy(h_tab + all, r.lens.data(), (size_t)all * 4);
        hipError_t e = hipSuccess;
        if (r.bytes) e = hipMemcpyAsync(s.d_arena.get(), s.stage.get(), r.bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tab, h_tab, (size_t)all * 8, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && call.totals.rounds) e = hipStreamWaitEvent(s.stream, mf.chain, 0);
        if (const int injected = e == hipSuccess ? injected_launch_failure(c, who) : 0) return injected;
        if (e == hipSuccess && m)
            e = vx::launch_merkle_blocks(s.d_arena.get(), d_tab, d_tab + all, m, d_window, s.stream);
        if (e == hipSuccess && r.hole_blocks)
            e = vx::launch_merkle_zero_leaves(d_tab + m, d_tab + all + m, r.hole_blocks, d_window,
                                              c->holes.zero_leaf, s.stream);
        for (const vx_merkle::Nodes& g : r.nodes) {
            if (e != hipSuccess) break;
            const uint64_t k = g.first - first;
            e = vx::launch_merkle_nodes(d_window + (size_t)g.row0 * 32, d_lw + k, g.n, g.log2_width,
                                        hashing ? d_exp + k * 32 : nullptr, hashing ? nullptr : d_exp + k * 32,
                                        hashing ? nullptr : d_match + k, s.stream);
            if (!lt || e != hipSuccess) continue;
            // the group's leaf rows out to the table, or against it: the bits, and the stored
            // rows into the shadow window, which must reduce to the same expected rows
            e = vx::launch_merkle_leaf_check(d_window, g.row0, g.n, g.log2_width, wpp, d_first + k, d_blocks + k,
                                             checking ? d_leaf : nullptr, checking ? d_bad + k * wpp : nullptr,
                                             checking ? d_shadow : nullptr, checking ? nullptr : d_leaf,
                                             s.stream);
            if (checking && e == hipSuccess)
                e = vx::launch_merkle_nodes(d_shadow + (size_t)g.row0 * 32, d_lw + k, g.n, g.log2_width, nullptr,
                                            d_exp + k * 32, d_layer_ok + k, s.stream);
        }
        if (e == hipSuccess) e = hipEventRecord(mf.chain, s.stream);
        if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
        if (e != hipSuccess) return hip_fail(e, (who + ": enqueue").c_str());
        c->holes.last.hole_blocks += r.hole_blocks;
        c->holes.last.hole_bytes += r.hole_bytes;
        return 0;
    };
    vx_files::Readers& rd = call.readers(io_threads, piece_length);
    vx_merkle::Rounds pack(file_lengths, nfiles, piece_length, first, count, bpr, R, entries, kMerkleRunBlocks,
                           in_hole);
    rc = vx_block_rounds::run<vx_merkle::Round>(pack, rd, c->slots.size(), call, enqueue, call.totals);
    call.sync_slots(rc);
    std::vector<uint8_t> verdict(hashing ? 0 : count);
    if (!rc && !hashing && hipMemcpy(verdict.data(), d_match, count, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(VX_EDEVICE, who + ": verdict download failed");
    if (!rc && hashing && hipMemcpy(rows_out, d_exp, count * 32, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(VX_EDEVICE, who + ": row download failed");
    if (!rc && tree_out)  // (the whole torrent: first == 0, count == n_pieces)
        rc = file_trees(c, d_exp, file_lengths, nfiles, piece_length, call.bad, tree_out, c->slots[0].stream, who);
    uint8_t* const leaves = lt && hashing ? lt->leaves_out + lr.base * 32 : nullptr;  // the range's rows
    if (!rc && leaves && hipMemcpy(leaves, d_leaf, lr.rows * 32, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(VX_EDEVICE, who + ": leaf table download failed");
    std::vector<uint8_t> layer_ok(checking ? count : 0);
    if (!rc && checking &&
        (hipMemcpy(lt->bad_out, d_bad, words * 8, hipMemcpyDeviceToHost) != hipSuccess ||
         hipMemcpy(layer_ok.data(), d_layer_ok, count, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(VX_EDEVICE, who + ": bitmap download failed");
    call.trace((uint64_t)bpr * VX_MERKLE_BLOCK);
    uint64_t mism = 0;
    for (size_t i = 0; i < count && !rc; ++i) {
        if (hashing) {  // never a row over bytes that were not read
            if (matched_out) matched_out[i] = !call.bad[i];
            if (call.bad[i]) std::memset(rows_out + i * 32, 0, 32);
            if (call.bad[i] && leaves)
                std::memset(leaves + (size_t)lr.leaf_first[i] * 32, 0, (size_t)lr.blocks[i] * 32);
            continue;
        }
        matched_out[i] = verdict[i] && !call.bad[i] ? 1 : 0;
        mism += !verdict[i] && !call.bad[i];  // I/O errors count in io_errors only
        if (!checking) continue;
        uint64_t* w = lt->bad_out + i * wpp;
        if (call.bad[i])  // it lacks bytes: every block it has is to be fetched
            for (uint32_t b = 0; b < wpp * 64; b += 64)
                w[b >> 6] = b + 64 <= lr.blocks[i] ? ~0ull : b < lr.blocks[i] ? (1ull << (lr.blocks[i] - b)) - 1 : 0;
        if (lt->layer_ok_out) lt->layer_ok_out[i] = layer_ok[i];
        if (lt->bad_counts_out) {
            uint32_t bits = 0;
            for (uint32_t k = 0; k < wpp; ++k) bits += (uint32_t)__builtin_popcountll(w[k]);
            lt->bad_counts_out[i] = bits;
        }
    }
    return call.end(rc, mism);
}

extern "C" {

int64_t vx_merkle_hash_files_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                                   uint32_t piece_length, size_t n_pieces, size_t first, size_t count,
                                   uint8_t* rows_out, uint8_t* ok_out, uint32_t io_threads) {
    if (!rows_out) return fail(VX_EINVAL, "vx_merkle_hash_files: NULL rows_out");
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, n_pieces, first, count, ok_out,
                             io_threads, rows_out);
}

int64_t vx_merkle_hash_files(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                             uint32_t piece_length, size_t n_pieces, uint8_t* rows_out, uint8_t* ok_out,
                             uint8_t* tree_out, uint64_t tree_rows, uint32_t io_threads) {
    if (!rows_out) return fail(VX_EINVAL, "vx_merkle_hash_files: NULL rows_out");
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, n_pieces, 0, n_pieces, ok_out,
                             io_threads, rows_out, tree_out, tree_rows);
}

int64_t vx_merkle_verify_files_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                                     uint32_t piece_length, const uint8_t* expected, size_t n_pieces, size_t first,
                                     size_t count, uint8_t* matched_out, uint32_t io_threads) {
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces, first, count,
                             matched_out, io_threads);
}

int64_t vx_merkle_verify_files(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths, size_t nfiles,
                               uint32_t piece_length, const uint8_t* expected, size_t n_pieces, uint8_t* matched_out,
                               uint32_t io_threads) {
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces, 0, n_pieces,
                             matched_out, io_threads);
}

int64_t vx_merkle_leaf_rows(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length) {
    if (nfiles && !file_lengths) return fail(VX_EINVAL, "vx_merkle_leaf_rows: NULL file_lengths");
    if (piece_length < VX_MERKLE_BLOCK || (piece_length & (piece_length - 1)))
        return fail(VX_EINVAL, "vx_merkle_leaf_rows: piece_length must be a power of two >= 16384");
    return (int64_t)vx_merkle::torrent_leaf_rows(file_lengths, nfiles);
}

int vx_merkle_device_leaf_check(const void* d_window, uint32_t row0, uint32_t n, uint32_t log2_width, uint32_t wpp,
                                const uint32_t* d_leaf_first, const uint32_t* d_blocks,
                                const void* d_expected_leaves, uint64_t* d_bad, void* d_shadow_out,
                                void* d_leaves_out, void* stream) {
    if (n == 0) return 0;
    const std::string who = "vx_merkle_device_leaf_check";
    if (!d_window || !d_leaf_first || !d_blocks)
        return fail(VX_EINVAL, who + ": NULL d_window, d_leaf_first or d_blocks");
    if (!d_expected_leaves != !d_bad)
        return fail(VX_EINVAL, who + ": d_expected_leaves and d_bad are given together or not at all");
    if (!d_expected_leaves && !d_leaves_out)
        return fail(VX_EINVAL, who + (d_shadow_out ? ": d_shadow_out needs d_expected_leaves"
                                                   : ": neither a bitmap nor d_leaves_out asked for"));
    if (log2_width > VX_MERKLE_MAX_LOG2_WIDTH) return fail(VX_EINVAL, who + ": log2_width > 17");
    if ((((uint64_t)n << log2_width) + row0) >> 32)
        return fail(VX_EINVAL, who + ": row0 + (n << log2_width) does not fit 32 bits");
    if (wpp < std::max<uint32_t>(1, (1u << log2_width) / 64))
        return fail(VX_EINVAL, who + ": wpp below max(1, 2^log2_width / 64)");
    if ((reinterpret_cast<uintptr_t>(d_window) | reinterpret_cast<uintptr_t>(d_expected_leaves) |
         reinterpret_cast<uintptr_t>(d_shadow_out) | reinterpret_cast<uintptr_t>(d_leaves_out)) & 15)
        return fail(VX_EINVAL, who + ": the row buffers must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_bad) & 7) ||
        ((reinterpret_cast<uintptr_t>(d_leaf_first) | reinterpret_cast<uintptr_t>(d_blocks)) & 3))
        return fail(VX_EINVAL, who + ": d_bad must be 8-byte, d_leaf_first and d_blocks 4-byte aligned");
    if (d_leaves_out && d_leaves_out == d_expected_leaves)
        return fail(VX_EINVAL, who + ": d_leaves_out and d_expected_leaves are one buffer");
    hipError_t e = vx::launch_merkle_leaf_check(
        static_cast<const uint8_t*>(d_window), row0, n, log2_width, wpp, d_leaf_first, d_blocks,
        static_cast<const uint8_t*>(d_expected_leaves), d_bad, static_cast<uint8_t*>(d_shadow_out),
        static_cast<uint8_t*>(d_leaves_out), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "merkle leaf check kernel launch");
    return 0;
}

int64_t vx_merkle_verify_files_blocks_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths,
                                            size_t nfiles, uint32_t piece_length, const uint8_t* expected,
                                            size_t n_pieces, const uint8_t* expected_leaves, uint64_t leaf_rows,
                                            size_t first, size_t count, uint8_t* matched_out, uint8_t* layer_ok_out,
                                            uint64_t* bad_out, uint32_t* bad_counts_out, uint32_t io_threads) {
    const LeafTable lt{expected_leaves, nullptr, leaf_rows, layer_ok_out, bad_out, bad_counts_out};
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces, first, count,
                             matched_out, io_threads, nullptr, nullptr, 0, &lt);
}

int64_t vx_merkle_verify_files_blocks(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths,
                                      size_t nfiles, uint32_t piece_length, const uint8_t* expected, size_t n_pieces,
                                      const uint8_t* expected_leaves, uint64_t leaf_rows, uint8_t* matched_out,
                                      uint8_t* layer_ok_out, uint64_t* bad_out, uint32_t* bad_counts_out,
                                      uint32_t io_threads) {
    return vx_merkle_verify_files_blocks_range(c, paths, file_lengths, nfiles, piece_length, expected, n_pieces,
                                               expected_leaves, leaf_rows, 0, n_pieces, matched_out, layer_ok_out,
                                               bad_out, bad_counts_out, io_threads);
}

int64_t vx_merkle_hash_files_leaves_range(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths,
                                          size_t nfiles, uint32_t piece_length, size_t n_pieces, size_t first,
                                          size_t count, uint8_t* rows_out, uint8_t* ok_out, uint8_t* leaves_out,
                                          uint64_t leaf_rows, uint32_t io_threads) {
    if (!rows_out) return fail(VX_EINVAL, "vx_merkle_hash_files_leaves: NULL rows_out");
    const LeafTable lt{nullptr, leaves_out, leaf_rows};
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, n_pieces, first, count, ok_out,
                             io_threads, rows_out, nullptr, 0, &lt);
}

int64_t vx_merkle_hash_files_leaves(vx_ctx* c, const char* const* paths, const uint64_t* file_lengths,
                                    size_t nfiles, uint32_t piece_length, size_t n_pieces, uint8_t* rows_out,
                                    uint8_t* ok_out, uint8_t* tree_out, uint64_t tree_rows, uint8_t* leaves_out,
                                    uint64_t leaf_rows, uint32_t io_threads) {
    if (!rows_out) return fail(VX_EINVAL, "vx_merkle_hash_files_leaves: NULL rows_out");
    const LeafTable lt{nullptr, leaves_out, leaf_rows};
    return merkle_files_impl(c, paths, file_lengths, nfiles, piece_length, nullptr, n_pieces, 0, n_pieces, ok_out,
                             io_threads, rows_out, tree_out, tree_rows, &lt);
}

}  // extern "C"
