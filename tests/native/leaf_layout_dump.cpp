// leaf_layout_dump.cpp — CPU harness for the leaf-table layout of a v2 torrent
// (vortex_amd/csrc/vx_merkle_leaves.hpp) and the rounds the files calls run it
// over (vx_merkle_rounds.hpp), used by tests/test_merkle_leaves_cpu.py.  Not
// the product; no GPU.
//
// stdin: the torrent's file lengths, one per line.  argv: piece_length first
// count [blocks_per_round] (count < 0: to the torrent's end).  stdout:
//   T rows                     the whole table's rows
//   L ok base rows             the range (ok 0: 2^32 rows or more)
//   p leaf_first blocks        one per piece of the range
// and with blocks_per_round, per round of the engine's packer over the range:
//   R data_blocks
//   t row len                  one per table entry, in order
//   n first n log2_width row0  one per node launch
//   W window_rows              last
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vx_merkle_leaves.hpp"

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: leaf_layout_dump piece_length first count [blocks_per_round] < lengths\n");
        return 2;
    }
    const uint32_t pl = (uint32_t)std::strtoul(argv[1], nullptr, 0);
    const uint64_t first = std::strtoull(argv[2], nullptr, 0);
    const long long count_arg = std::strtoll(argv[3], nullptr, 0);
    const uint32_t bpr = argc > 4 ? (uint32_t)std::strtoul(argv[4], nullptr, 0) : 0;
    std::vector<uint64_t> lens;
    unsigned long long x;
    while (std::scanf("%llu", &x) == 1) lens.push_back(x);
    const uint64_t total = vx_merkle::torrent_pieces(lens.data(), lens.size(), pl);
    if (first > total) return 3;
    const uint64_t count = count_arg < 0 ? total - first : (uint64_t)count_arg;
    if (count > total - first) return 3;

    std::printf("T %llu\n", (unsigned long long)vx_merkle::torrent_leaf_rows(lens.data(), lens.size()));
    vx_merkle::LeafRange lr;
    const bool ok = vx_merkle::leaf_range(lens.data(), lens.size(), pl, first, count, lr);
    std::printf("L %d %llu %llu\n", ok ? 1 : 0, (unsigned long long)lr.base, (unsigned long long)lr.rows);
    if (!ok) return 0;
    if (lr.leaf_first.size() != count || lr.blocks.size() != count) return 4;
    for (size_t k = 0; k < lr.blocks.size(); ++k) std::printf("p %u %u\n", lr.leaf_first[k], lr.blocks[k]);
    if (!bpr) return 0;

    const uint32_t window = vx_merkle::Rounds::window_for(bpr, pl);
    vx_merkle::Rounds pack(lens.data(), lens.size(), pl, first, count, bpr, window, 2 * bpr + pl / vx_merkle::kBlock,
                           128);
    vx_merkle::Round r;
    while (pack.next(r)) {
        std::printf("R %u\n", r.data_blocks);
        for (size_t k = 0; k < r.rows.size(); ++k) std::printf("t %u %u\n", r.rows[k], r.lens[k]);
        for (const auto& g : r.nodes)
            std::printf("n %llu %u %u %u\n", (unsigned long long)g.first, g.n, g.log2_width, g.row0);
    }
    std::printf("W %u\n", window);
    return 0;
}
