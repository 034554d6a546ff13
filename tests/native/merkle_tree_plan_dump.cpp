// merkle_tree_plan_dump — the host side of the layer trees
// (vortex_amd/csrc/vx_merkle_tree.hpp) as a stand-alone program, so the test
// can run it under ASan+UBSan without a GPU (tests/test_merkle_tree_cpu.py).
//
//   merkle_tree_plan_dump dump     counts on stdin, one per line; prints
//       "T pass src_row dst_row level_rows tile" per tile, "O tree_off" per
//       offset, then the plan as JSON.  The tile and offset arrays are exactly
//       as long as the plan says (heap), so a write past them is an ASan error.
//   merkle_tree_plan_dump errors   counts on stdin (a valid list); checks what
//       the planner, the layout and the proof lookup refuse and that a refused
//       call leaves its outputs untouched; prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vx_merkle_tree.hpp"

static int die(const char* what) {
    std::fprintf(stderr, "merkle_tree_plan_dump: %s\n", what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 2) return die("usage: merkle_tree_plan_dump dump|errors < counts");
    std::vector<uint32_t> counts;
    unsigned long long v;
    while (std::scanf("%llu", &v) == 1) counts.push_back((uint32_t)v);
    const uint32_t n = (uint32_t)counts.size();
    struct vx_merkle_tree_plan plan;
    if (!std::strcmp(argv[1], "dump")) {
        if (vx_merkle::plan_trees(counts.data(), n, &plan, nullptr, 0, nullptr)) return die("the counts were refused");
        vx_merkle_tree_tile* tiles =
            static_cast<vx_merkle_tree_tile*>(std::malloc(sizeof(vx_merkle_tree_tile) * (plan.n_tiles + !plan.n_tiles)));
        uint64_t* off = static_cast<uint64_t*>(std::malloc(sizeof(uint64_t) * ((size_t)n + 1)));
        struct vx_merkle_tree_plan again;
        if (vx_merkle::plan_trees(counts.data(), n, &again, tiles, plan.n_tiles, off)) return die("refused with tiles");
        if (std::memcmp(&plan, &again, sizeof plan)) return die("the plan differs between the two calls");
        uint32_t t = 0;
        for (uint32_t p = 0; p < plan.passes; ++p)
            for (uint32_t k = 0; k < plan.pass_tiles[p]; ++k, ++t)
                std::printf("T %u %u %u %u %u\n", p, tiles[t].src_row, tiles[t].dst_row, tiles[t].level_rows,
                            tiles[t].tile);
        for (uint32_t f = 0; f <= n; ++f) std::printf("O %llu\n", (unsigned long long)off[f]);
        std::printf("{\"n_layers\": %u, \"passes\": %u, \"rows\": %llu, \"tree_rows\": %llu, \"n_tiles\": %u, "
                    "\"pass_tiles\": [%u, %u, %u, %u]}\n",
                    plan.n_layers, plan.passes, (unsigned long long)plan.rows, (unsigned long long)plan.tree_rows,
                    plan.n_tiles, plan.pass_tiles[0], plan.pass_tiles[1], plan.pass_tiles[2], plan.pass_tiles[3]);
        std::free(tiles);
        std::free(off);
        return 0;
    }
    if (std::strcmp(argv[1], "errors")) return die("unknown mode");
    if (n < 2 || vx_merkle::plan_trees(counts.data(), n, &plan, nullptr, 0, nullptr) || plan.n_tiles < 2)
        return die("errors needs a valid list of at least two counts");
    // tiles_cap = n_tiles - 1: refused, and neither the array, the guard behind it nor tree_off is touched
    const size_t guard = 64, cap = plan.n_tiles - 1;
    std::vector<uint8_t> buf((cap + guard) * sizeof(vx_merkle_tree_tile), 0xA5);
    std::vector<uint64_t> off((size_t)n + 1 + guard, 0xA5A5A5A5A5A5A5A5ull);
    struct vx_merkle_tree_plan out;
    vx_merkle_tree_tile* tiles = reinterpret_cast<vx_merkle_tree_tile*>(buf.data());
    if (vx_merkle::plan_trees(counts.data(), n, &out, tiles, cap, off.data()) != VX_EINVAL)
        return die("tiles_cap = n_tiles - 1 was accepted");
    for (uint8_t b : buf)
        if (b != 0xA5) return die("a refused call wrote to tiles");
    for (uint64_t o : off)
        if (o != 0xA5A5A5A5A5A5A5A5ull) return die("a refused call wrote to tree_off");
    // ... and with tiles_cap = n_tiles the guards stay as they were
    if (vx_merkle::plan_trees(counts.data(), n, &out, tiles, cap + 1, off.data())) return die("tiles_cap = n_tiles was refused");
    for (size_t k = (cap + 1) * sizeof(vx_merkle_tree_tile); k < buf.size(); ++k)
        if (buf[k] != 0xA5) return die("the planner wrote past n_tiles");
    for (size_t k = (size_t)n + 1; k < off.size(); ++k)
        if (off[k] != 0xA5A5A5A5A5A5A5A5ull) return die("the planner wrote past tree_off[n_layers]");
    if (off[n] != out.tree_rows) return die("tree_off[n_layers] is not tree_rows");
    // a zero count, anywhere
    for (uint32_t at : {0u, n / 2, n - 1}) {
        std::vector<uint32_t> c = counts;
        c[at] = 0;
        if (vx_merkle::plan_trees(c.data(), n, &out, nullptr, 0, nullptr) != VX_EINVAL) return die("a zero count was accepted");
    }
    // 2^32 rows in the layers, or in the trees (2^31 + 1 rows make a tree of 2^32 + 32 rows): refused
    const uint32_t half[2] = {0x80000000u, 0x80000000u}, big = 0x80000001u, fits = 0x7FFFFFF0u;
    if (vx_merkle::plan_trees(half, 2, &out, nullptr, 0, nullptr) != VX_EINVAL) return die("a sum of 2^32 was accepted");
    if (vx_merkle::plan_trees(&big, 1, &out, nullptr, 0, nullptr) != VX_EINVAL) return die("a tree of 2^32 rows was accepted");
    if (vx_merkle::plan_trees(&fits, 1, &out, nullptr, 0, nullptr) || out.passes != 4 || out.pass_tiles[3] != 1 ||
        out.tree_rows != vx_merkle::tree_rows(fits) || (out.tree_rows >> 32))
        return die("one layer of 2^31 - 16 rows must take four passes");
    // no layers: an empty plan
    uint64_t none = 7;
    if (vx_merkle::plan_trees(nullptr, 0, &out, nullptr, 0, &none) || out.passes || out.n_tiles || out.rows ||
        out.tree_rows || none != 0)
        return die("no layers must give an empty plan");
    if (vx_merkle::plan_trees(counts.data(), n, nullptr, nullptr, 0, nullptr) != VX_EINVAL) return die("a NULL plan was accepted");
    // the layout of a torrent: empty files, a file of exactly piece_length, one byte more
    const uint64_t flens[5] = {0, 65536, 65537, 1, 3 * 65536};
    uint32_t lc[5];
    uint64_t lo[6];
    if (vx_merkle::tree_layout(flens, 5, 65536, lc, lo) != 1 + 3 + 1 + 6 || lc[0] != 0 || lc[1] != 1 || lc[2] != 2 ||
        lc[3] != 1 || lc[4] != 3 || lo[0] != 0 || lo[1] != 0 || lo[2] != 1 || lo[3] != 4 || lo[4] != 5 || lo[5] != 11)
        return die("the layout of five files is wrong");
    const uint64_t huge = ~0ull - 65536;
    if (vx_merkle::tree_layout(&huge, 1, 16384, lc, lo) != -1) return die("a file of 2^32 pieces or more was accepted");
    // the proof lookup: a tree of exactly tree_rows(5) rows and an output of exactly (span + uncles) rows
    // on the heap, so a read or write past either is an ASan error
    const uint32_t m = 5;
    const size_t trows = (size_t)vx_merkle::tree_rows(m);
    if (trows != 5 + 3 + 2 + 1) return die("tree_rows(5) is not 11");
    std::vector<uint8_t> pads((size_t)vx_merkle::kProofPads * 32);
    for (size_t k = 0; k < pads.size(); ++k) pads[k] = (uint8_t)(k / 32);  // pad(h) stands as 32 bytes of h
    uint8_t* tree = static_cast<uint8_t*>(std::malloc(trows * 32));
    for (size_t k = 0; k < trows * 32; ++k) tree[k] = (uint8_t)(0x80 + k / 32);  // row r as 32 bytes of 0x80 + r
    for (uint32_t span : {1u, 2u, 4u, 8u, 512u})
        for (uint32_t uncles : {0u, 1u, 3u, 64u}) {
            uint8_t* o = static_cast<uint8_t*>(std::malloc((size_t)(span + uncles) * 32 + !(span + uncles)));
            if (vx_merkle::tree_proof(tree, m, 64, 0, 0, span, uncles, pads.data(), o)) return die("a proof was refused");
            if (o[0] != 0x80) return die("the span's first row is not row 0 of the tree");
            if (span == 8 && o[5 * 32] != 64) return die("a row past the layer is not the pad hash of its height");
            if (span == 1 && uncles && o[32] != 0x81) return die("the first uncle of row 0 is not row 1");
            if (span == 4 && uncles && o[4 * 32] != 0x80 + 9) return die("the uncle of span 0 of 4 is not level 2 row 1");
            if (span == 8 && uncles && o[8 * 32] != 64 + 3) return die("an uncle above the root is not a pad hash");
            std::free(o);
        }
    uint8_t o[40 * 32];
    const struct {
        uint32_t level, span, uncles;
        uint64_t pos;
    } bad[] = {{0, 0, 0, 0}, {0, 3, 0, 0}, {0, 1024, 0, 0}, {0, 1, 65, 0}, {4, 1, 0, 0}, {0, 1, 0, 5}, {0, 4, 0, 2},
               {3, 1, 0, 1}, {0, 1, 0, ~0ull}};
    for (const auto& b : bad)
        if (vx_merkle::tree_proof(tree, m, 0, b.level, b.pos, b.span, b.uncles, pads.data(), o) != VX_EINVAL)
            return die("a bad proof request was accepted");
    if (vx_merkle::tree_proof(tree, 0, 0, 0, 0, 1, 0, pads.data(), o) != VX_EINVAL ||
        vx_merkle::tree_proof(tree, m, 65, 0, 0, 1, 0, pads.data(), o) != VX_EINVAL ||
        vx_merkle::tree_proof(nullptr, m, 0, 0, 0, 1, 0, pads.data(), o) != VX_EINVAL)
        return die("m == 0, height > 64 or a NULL tree was accepted");
    if (vx_merkle::tree_proof(tree, m, 0, 3, 0, 1, 2, pads.data(), o) || o[0] != 0x80 + 10 || o[32] != 3 || o[64] != 4)
        return die("the root's own proof is wrong");
    std::free(tree);
    std::puts("ok");
    return 0;
}
