// hybrid_rounds_dump.cpp — CPU harness for the hybrid re-verify's round planner
// (vortex_amd/csrc/vx_hybrid_rounds.hpp), used by tests/test_hybrid_cpu.py.
// Not the product; no GPU.
//
// stdin: the torrent's file lengths (real files only), one per line.  argv:
// piece_length first count stage_bytes [chunk row_budget quiet] (count < 0: to
// the torrent's end; chunk / row_budget 0: the engine's choice).  stdout, per
// round:
//   R new_window end_window w_first w_n w_log2 data_blocks bytes file_bytes
//   r file file_off len stage_off piece          one per read
//   l stage_off len pid poff tlen                one per SHA-1 lane
//   z tail_off data_len pad_len pid              one per tail lane
//   t row len                                    one per block-table entry, in order
// then a JSON summary line.  quiet = 1 prints the summary only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vx_hybrid_rounds.hpp"

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: hybrid_rounds_dump piece_length first count stage_bytes "
                             "[chunk row_budget quiet] < lengths\n");
        return 2;
    }
    using ull = unsigned long long;
    const uint32_t pl = (uint32_t)std::strtoul(argv[1], nullptr, 0);
    const uint64_t first = std::strtoull(argv[2], nullptr, 0);
    const long long count_arg = std::strtoll(argv[3], nullptr, 0);
    const uint64_t stage = std::strtoull(argv[4], nullptr, 0) / vx_hybrid::kBlock * vx_hybrid::kBlock;
    uint64_t chunk = argc > 5 ? std::strtoull(argv[5], nullptr, 0) : 0;
    uint32_t budget = argc > 6 ? (uint32_t)std::strtoul(argv[6], nullptr, 0) : 0;
    const bool quiet = argc > 7 && std::atoi(argv[7]) != 0;
    std::vector<uint64_t> lens;
    ull x;
    while (std::scanf("%llu", &x) == 1) lens.push_back(x);
    const uint64_t total = vx_merkle::torrent_pieces(lens.data(), lens.size(), pl);
    if (first > total) return 3;
    const uint64_t count = count_arg < 0 ? total - first : (uint64_t)count_arg;
    if (count > total - first) return 3;
    chunk = vx_hybrid::chunk_for(pl, stage, chunk ? chunk : vx_hybrid::kChunk);
    if (chunk == 0) return 4;
    if (!budget) budget = vx_hybrid::kRowBudget;

    vx_hybrid::Rounds plan(lens.data(), lens.size(), pl, total, first, count, stage, chunk, budget);
    vx_hybrid::Round r;
    ull rounds = 0, windows = 0, lanes = 0, tails = 0, entries = 0, max_entries = 0, max_rows = 0;
    while (plan.next(r)) {
        ++rounds;
        windows += r.new_window;
        lanes += r.l_len.size();
        tails += r.t_len.size();
        entries += r.rows.size();
        max_entries = r.rows.size() > max_entries ? r.rows.size() : max_entries;
        const ull wrows = (ull)r.w_n << r.w_log2;
        max_rows = wrows > max_rows ? wrows : max_rows;
        if (quiet) continue;
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
    }
    std::printf("{\"files\": %zu, \"pieces\": %llu, \"rounds\": %llu, \"windows\": %llu, \"lanes\": %llu, "
                "\"tails\": %llu, \"entries\": %llu, \"max_entries\": %llu, \"max_window_rows\": %llu, "
                "\"chunk\": %llu, \"row_budget\": %u}\n",
                lens.size(), (ull)total, rounds, windows, lanes, tails, entries, max_entries, max_rows, (ull)chunk,
                budget);
    return 0;
}
