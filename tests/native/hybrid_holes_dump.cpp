// hybrid_holes_dump.cpp — CPU harness for the hybrid re-verify's round planner
// over file holes (vortex_amd/csrc/vx_hybrid_rounds.hpp with the scan of
// vx_extents.hpp as its hole predicate), used by
// tests/test_hybrid_sparse_cpu.py.  Not the product; no GPU.
//
// stdin: the torrent's files, one per line: "length path" (a path that does
// not open is a missing file).  argv:
//   mode piece_length first count stage_bytes [chunk row_budget]
// mode: none (no predicate), false (a predicate that is never true), holes (the
// scan).  count < 0: to the torrent's end; chunk / row_budget 0: the engine's
// choice.  stdout, per round, the lines of hybrid_rounds_dump.cpp
//   R new_window end_window w_first w_n w_log2 data_blocks bytes file_bytes
//   r file file_off len stage_off piece          one per read
//   l stage_off len pid poff tlen                one per SHA-1 lane
//   z tail_off data_len pad_len pid              one per tail lane
//   t row len                                    one per block-table entry, in order:
//                                                data blocks, absent slots, hole blocks
// and, only where there is something to say,
//   H hole_blocks hole_bytes                     the round's hole chunks
//   h pid poff blocks                            one per zero-run lane
//   w pid total_len                              one per whole-hole piece of the window (first round)
// then a JSON summary line.
#include <fcntl.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "vx_extents.hpp"
#include "vx_hybrid_rounds.hpp"

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: hybrid_holes_dump none|false|holes piece_length first count stage_bytes "
                             "[chunk row_budget] < files\n");
        return 2;
    }
    using ull = unsigned long long;
    const std::string mode = argv[1];
    const uint32_t pl = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint64_t first = std::strtoull(argv[3], nullptr, 0);
    const long long count_arg = std::strtoll(argv[4], nullptr, 0);
    const uint64_t stage = std::strtoull(argv[5], nullptr, 0) / vx_hybrid::kBlock * vx_hybrid::kBlock;
    uint64_t chunk = argc > 6 ? std::strtoull(argv[6], nullptr, 0) : 0;
    uint32_t budget = argc > 7 ? (uint32_t)std::strtoul(argv[7], nullptr, 0) : 0;
    std::vector<uint64_t> lens;
    std::vector<std::string> paths;
    for (std::string line; std::getline(std::cin, line);) {
        const size_t sp = line.find(' ');
        if (sp == std::string::npos) continue;
        lens.push_back(std::strtoull(line.substr(0, sp).c_str(), nullptr, 0));
        paths.push_back(line.substr(sp + 1));
    }
    const uint64_t total = vx_merkle::torrent_pieces(lens.data(), lens.size(), pl);
    if (first > total) return 3;
    const uint64_t count = count_arg < 0 ? total - first : (uint64_t)count_arg;
    if (count > total - first) return 3;
    chunk = vx_hybrid::chunk_for(pl, stage, chunk ? chunk : vx_hybrid::kChunk);
    if (chunk == 0) return 4;
    if (!budget) budget = vx_hybrid::kRowBudget;

    std::vector<int> fds(paths.size(), -1);
    if (mode == "holes")
        for (size_t f = 0; f < paths.size(); ++f) fds[f] = open(paths[f].c_str(), O_RDONLY | O_CLOEXEC);
    const vx_extents::Holes holes = mode == "holes" ? vx_extents::Holes(fds, lens.data()) : vx_extents::Holes();
    vx_merkle::HolePredicate pred;
    if (mode == "holes")
        pred = [&holes](uint32_t f, uint64_t off, uint32_t len) { return holes.hole(f, (int64_t)off, len); };
    else if (mode == "false")
        pred = [](uint32_t, uint64_t, uint32_t) { return false; };
    else if (mode != "none")
        return 2;

    vx_hybrid::Rounds plan(lens.data(), lens.size(), pl, total, first, count, stage, chunk, budget, vx_hybrid::kMaxRun,
                           pred);
    vx_hybrid::Round r;
    ull rounds = 0, windows = 0, lanes = 0, tails = 0, entries = 0, max_entries = 0, max_rows = 0;
    ull zero_runs = 0, hole_pieces = 0, hole_blocks = 0, hole_bytes = 0, file_bytes = 0;
    while (plan.next(r)) {
        ++rounds;
        windows += r.new_window;
        lanes += r.l_len.size();
        tails += r.t_len.size();
        entries += r.rows.size();
        max_entries = r.rows.size() > max_entries ? r.rows.size() : max_entries;
        const ull wrows = (ull)r.w_n << r.w_log2;
        max_rows = wrows > max_rows ? wrows : max_rows;
        zero_runs += r.z_pid.size();
        hole_pieces += r.hole_pid.size();
        hole_blocks += r.hole_blocks;
        hole_bytes += r.hole_bytes;
        file_bytes += r.file_bytes;
        std::printf("R %d %d %llu %u %u %u %llu %llu\n", (int)r.new_window, (int)r.end_window, (ull)r.w_first, r.w_n,
                    r.w_log2, r.data_blocks, (ull)r.bytes, (ull)r.file_bytes);
        for (const auto& it : r.reads)
            std::printf("r %u %llu %llu %llu %llu\n", it.file, (ull)it.file_off, (ull)it.len, (ull)it.stage_off,
                        (ull)it.piece);
        for (size_t k = 0; k < r.l_len.size(); ++k)
            std::printf("l %llu %u %u %llu %llu\n", (ull)r.l_off[k], r.l_len[k], r.l_pid[k], (ull)r.l_poff[k],
                        (ull)r.l_tlen[k]);
        for (size_t k = 0; k < r.t_len.size(); ++k)
            std::printf("z %llu %u %u %u\n", (ull)r.t_off[k], r.t_len[k], r.t_pad[k], r.t_pid[k]);
        for (size_t k = 0; k < r.rows.size(); ++k) std::printf("t %u %u\n", r.rows[k], r.lens[k]);
        if (r.hole_blocks || r.hole_bytes) std::printf("H %u %llu\n", r.hole_blocks, (ull)r.hole_bytes);
        for (size_t k = 0; k < r.z_pid.size(); ++k) std::printf("h %u %u %u\n", r.z_pid[k], r.z_poff[k], r.z_blocks[k]);
        for (size_t k = 0; k < r.hole_pid.size(); ++k) std::printf("w %u %u\n", r.hole_pid[k], r.hole_len[k]);
    }
    std::printf("{\"files\": %zu, \"pieces\": %llu, \"rounds\": %llu, \"windows\": %llu, \"lanes\": %llu, "
                "\"tails\": %llu, \"entries\": %llu, \"max_entries\": %llu, \"max_window_rows\": %llu, "
                "\"chunk\": %llu, \"row_budget\": %u, \"extents\": %llu, \"zero_runs\": %llu, \"hole_pieces\": %llu, "
                "\"hole_blocks\": %llu, \"hole_bytes\": %llu, \"file_bytes\": %llu}\n",
                lens.size(), (ull)total, rounds, windows, lanes, tails, entries, max_entries, max_rows, (ull)chunk,
                budget, (ull)holes.extents(), zero_runs, hole_pieces, hole_blocks, hole_bytes, file_bytes);
    for (int fd : fds)
        if (fd >= 0) close(fd);
    return 0;
}
