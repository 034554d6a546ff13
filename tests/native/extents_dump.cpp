// extents_dump.cpp — CPU harness for the re-verify over file holes
// (vortex_amd/csrc/vx_extents.hpp and the hole predicate of
// vx_merkle_rounds.hpp), used by tests/test_sparse_cpu.py.  Not the product;
// no GPU.
//
// stdin: the torrent's files, one per line: "length path" (a path that does
// not open is a missing file).  argv:
//   v1 piece_length cap
//   v2 piece_length cap first count blocks_per_round [window_rows max_entries max_run_blocks]
// (cap: extents scanned per file; count < 0: to the torrent's end; window_rows
// / max_entries 0: the engine's choice).  stdout, both modes:
//   F file bound extents                         one per file, then
//   e lo hi                                      one per data extent of it
// v1 then prints "P piece hole" per piece (hole: every segment lies wholly in
// holes); v2 prints the packer's rounds with the scan as its hole predicate:
//   R data_blocks bytes file_bytes hole_blocks hole_bytes
//   r file file_off len stage_block piece        one per read
//   t row len                                    one per table entry, in order:
//                                                data blocks, absent slots, hole blocks
//   n first n log2_width row0                    one per node launch
// and both end with a JSON summary line.
#include <fcntl.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "vx_extents.hpp"
#include "vx_merkle_rounds.hpp"

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: extents_dump v1|v2 piece_length cap [first count blocks_per_round "
                             "[window_rows max_entries max_run_blocks]] < files\n");
        return 2;
    }
    const std::string mode = argv[1];
    const uint32_t pl = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const size_t cap = (size_t)std::strtoull(argv[3], nullptr, 0);
    std::vector<uint64_t> lens;
    std::vector<std::string> paths;
    for (std::string line; std::getline(std::cin, line);) {
        const size_t sp = line.find(' ');
        if (sp == std::string::npos) continue;
        lens.push_back(std::strtoull(line.substr(0, sp).c_str(), nullptr, 0));
        paths.push_back(line.substr(sp + 1));
    }
    std::vector<int> fds(paths.size(), -1);
    for (size_t f = 0; f < paths.size(); ++f) fds[f] = open(paths[f].c_str(), O_RDONLY | O_CLOEXEC);
    const vx_extents::Holes holes(fds, lens.data(), cap);
    for (size_t f = 0; f < fds.size(); ++f) {
        const vx_extents::File& x = holes.file(f);
        std::printf("F %zu %lld %zu\n", f, (long long)x.bound, x.data.size());
        for (const vx_extents::Extent& e : x.data) std::printf("e %lld %lld\n", (long long)e.lo, (long long)e.hi);
    }
    int rc = 0;
    if (mode == "v1") {
        uint64_t total = 0;
        for (uint64_t L : lens) total += L;
        const int64_t n = pl ? (int64_t)((total + pl - 1) / pl) : 0;
        const auto fs = vx_files::layout(lens.data(), lens.size(), pl);
        std::vector<vx_files::Seg> segs;
        uint64_t nh = 0;
        for (int64_t p = 0; p < n; ++p) {
            const bool h = holes.hole_piece(fs, p, pl, segs);
            nh += h;
            std::printf("P %lld %d\n", (long long)p, h ? 1 : 0);
        }
        std::printf("{\"files\": %zu, \"pieces\": %lld, \"extents\": %llu, \"any\": %d, \"hole_pieces\": %llu}\n",
                    lens.size(), (long long)n, (unsigned long long)holes.extents(), holes.any() ? 1 : 0,
                    (unsigned long long)nh);
    } else if (mode == "v2" && argc >= 7) {
        const uint64_t first = std::strtoull(argv[4], nullptr, 0);
        const long long count_arg = std::strtoll(argv[5], nullptr, 0);
        const uint32_t bpr = (uint32_t)std::strtoul(argv[6], nullptr, 0);
        uint32_t window = argc > 7 ? (uint32_t)std::strtoul(argv[7], nullptr, 0) : 0;
        uint32_t entries = argc > 8 ? (uint32_t)std::strtoul(argv[8], nullptr, 0) : 0;
        const uint32_t max_run = argc > 9 ? (uint32_t)std::strtoul(argv[9], nullptr, 0) : 128;
        const uint64_t total = vx_merkle::torrent_pieces(lens.data(), lens.size(), pl);
        if (first > total) return 3;
        const uint64_t count = count_arg < 0 ? total - first : (uint64_t)count_arg;
        if (count > total - first) return 3;
        if (!window) window = vx_merkle::Rounds::window_for(bpr, pl);
        if (!entries) entries = 2 * bpr + pl / vx_merkle::kBlock;
        vx_merkle::Rounds pack(lens.data(), lens.size(), pl, first, count, bpr, window, entries, max_run,
                               [&holes](uint32_t f, uint64_t off, uint32_t len) {
                                   return holes.hole(f, (int64_t)off, len);
                               });
        vx_merkle::Round r;
        uint64_t rounds = 0, blocks = 0, hole_blocks = 0, hole_bytes = 0;
        while (pack.next(r)) {
            ++rounds;
            blocks += r.data_blocks;
            hole_blocks += r.hole_blocks;
            hole_bytes += r.hole_bytes;
            std::printf("R %u %llu %llu %u %llu\n", r.data_blocks, (unsigned long long)r.bytes,
                        (unsigned long long)r.file_bytes, r.hole_blocks, (unsigned long long)r.hole_bytes);
            for (const auto& it : r.reads)
                std::printf("r %u %llu %llu %u %llu\n", it.file, (unsigned long long)it.file_off,
                            (unsigned long long)it.len, it.stage_block, (unsigned long long)it.piece);
            for (size_t k = 0; k < r.rows.size(); ++k) std::printf("t %u %u\n", r.rows[k], r.lens[k]);
            for (const auto& g : r.nodes)
                std::printf("n %llu %u %u %u\n", (unsigned long long)g.first, g.n, g.log2_width, g.row0);
        }
        std::printf("{\"files\": %zu, \"pieces\": %llu, \"extents\": %llu, \"rounds\": %llu, \"blocks\": %llu, "
                    "\"hole_blocks\": %llu, \"hole_bytes\": %llu, \"window_rows\": %u, \"max_entries\": %u}\n",
                    lens.size(), (unsigned long long)total, (unsigned long long)holes.extents(),
                    (unsigned long long)rounds, (unsigned long long)blocks, (unsigned long long)hole_blocks,
                    (unsigned long long)hole_bytes, window, entries);
    } else {
        rc = 2;
    }
    for (int fd : fds)
        if (fd >= 0) close(fd);
    return rc;
}
