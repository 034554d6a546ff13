// merkle_rounds_dump.cpp — CPU harness for the v2 re-verify's round packer
// (vortex_amd/csrc/vx_merkle_rounds.hpp), used by tests/test_merkle_files_cpu.py.
// Not the product; no GPU.
//
// stdin: the torrent's file lengths, one per line.  argv: piece_length first
// count blocks_per_round [window_rows max_entries max_run_blocks quiet]
// (count < 0: to the torrent's end; window_rows / max_entries 0: the engine's
// choice).  stdout, per round:
//   R data_blocks bytes file_bytes
//   r file file_off len stage_block piece        one per read
//   t row len                                    one per table entry, in order
//   n first n log2_width row0                    one per node launch
// then a JSON summary line.  quiet = 1 prints the summary only.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vx_merkle_rounds.hpp"

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: merkle_rounds_dump piece_length first count blocks_per_round "
                             "[window_rows max_entries max_run_blocks quiet] < lengths\n");
        return 2;
    }
    const uint32_t pl = (uint32_t)std::strtoul(argv[1], nullptr, 0);
    const uint64_t first = std::strtoull(argv[2], nullptr, 0);
    const long long count_arg = std::strtoll(argv[3], nullptr, 0);
    const uint32_t bpr = (uint32_t)std::strtoul(argv[4], nullptr, 0);
    uint32_t window = argc > 5 ? (uint32_t)std::strtoul(argv[5], nullptr, 0) : 0;
    uint32_t entries = argc > 6 ? (uint32_t)std::strtoul(argv[6], nullptr, 0) : 0;
    const uint32_t max_run = argc > 7 ? (uint32_t)std::strtoul(argv[7], nullptr, 0) : 256;
    const bool quiet = argc > 8 && std::atoi(argv[8]) != 0;
    std::vector<uint64_t> lens;
    unsigned long long x;
    while (std::scanf("%llu", &x) == 1) lens.push_back(x);
    const uint64_t total = vx_merkle::torrent_pieces(lens.data(), lens.size(), pl);
    if (first > total) return 3;
    const uint64_t count = count_arg < 0 ? total - first : (uint64_t)count_arg;
    if (count > total - first) return 3;
    if (!window) window = vx_merkle::Rounds::window_for(bpr, pl);
    if (!entries) entries = 2 * bpr + pl / vx_merkle::kBlock;

    const auto t0 = std::chrono::steady_clock::now();
    vx_merkle::Rounds pack(lens.data(), lens.size(), pl, first, count, bpr, window, entries, max_run);
    vx_merkle::Round r;
    uint64_t rounds = 0, blocks = 0, table = 0, launches = 0;
    while (pack.next(r)) {
        ++rounds;
        blocks += r.data_blocks;
        table += r.rows.size();
        launches += r.nodes.size();
        if (quiet) continue;
        std::printf("R %u %llu %llu\n", r.data_blocks, (unsigned long long)r.bytes, (unsigned long long)r.file_bytes);
        for (const auto& it : r.reads)
            std::printf("r %u %llu %llu %u %llu\n", it.file, (unsigned long long)it.file_off,
                        (unsigned long long)it.len, it.stage_block, (unsigned long long)it.piece);
        for (size_t k = 0; k < r.rows.size(); ++k) std::printf("t %u %u\n", r.rows[k], r.lens[k]);
        for (const auto& g : r.nodes)
            std::printf("n %llu %u %u %u\n", (unsigned long long)g.first, g.n, g.log2_width, g.row0);
    }
    const double build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"files\": %zu, \"pieces\": %llu, \"rounds\": %llu, \"blocks\": %llu, \"entries\": %llu, "
                "\"launches\": %llu, \"window_rows\": %u, \"max_entries\": %u, \"build_ms\": %.3f}\n",
                lens.size(), (unsigned long long)total, (unsigned long long)rounds, (unsigned long long)blocks,
                (unsigned long long)table, (unsigned long long)launches, window, entries, build_ms);
    return 0;
}
