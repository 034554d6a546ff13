// merkle_readers_check.cpp — CPU harness for the read side of the v2 re-verify
// (vx_merkle_rounds.hpp's rounds read by vx_files::Readers in `blocks` mode,
// with DirectIo), used by tests/test_merkle_files_cpu.py under ASan + UBSan.
// Not the product; no GPU.
//
// argv: dir piece_length blocks_per_round threads direct_io.  stdin: one line
// per file, "declared_length actual_length" (actual < 0: the file is missing).
// The program writes the files (byte p of file f is pattern(f, p)), reads every
// round into a stage of exactly blocks_per_round blocks, as the engine does,
// and checks each block of every piece that was not marked bad against the
// pattern.  stdout: a JSON line with the bad pieces and the mismatch count.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vx_files.hpp"
#include "vx_merkle_rounds.hpp"

static uint8_t pattern(size_t f, uint64_t p) { return (uint8_t)(p * 131 + f * 17 + (p >> 8) + (p >> 16)); }

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const std::string dir = argv[1];
    const uint32_t pl = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint32_t bpr = (uint32_t)std::strtoul(argv[3], nullptr, 0);
    const int threads = std::atoi(argv[4]);
    const bool direct = std::atoi(argv[5]) != 0;
    std::vector<uint64_t> lens;
    std::vector<long long> actual;
    unsigned long long a;
    long long b;
    while (std::scanf("%llu %lld", &a, &b) == 2) {
        lens.push_back(a);
        actual.push_back(b);
    }
    std::vector<int> fds(lens.size(), -1);
    for (size_t f = 0; f < lens.size(); ++f) {
        if (actual[f] < 0) continue;
        const std::string path = dir + "/f" + std::to_string(f);
        std::vector<uint8_t> body((size_t)actual[f]);
        for (size_t p = 0; p < body.size(); ++p) body[p] = pattern(f, p);
        FILE* out = std::fopen(path.c_str(), "wb");
        if (!out || (!body.empty() && std::fwrite(body.data(), 1, body.size(), out) != body.size())) return 3;
        std::fclose(out);
        fds[f] = open(path.c_str(), O_RDONLY | O_CLOEXEC);
    }
    const uint64_t n = vx_merkle::torrent_pieces(lens.data(), lens.size(), pl);
    std::vector<uint8_t> bad(n ? n : 1, 0);
    void* raw = nullptr;
    if (posix_memalign(&raw, 4096, (size_t)bpr * vx_merkle::kBlock)) return 3;
    uint8_t* stage = static_cast<uint8_t*>(raw);
    uint64_t mismatches = 0, rounds = 0;
    {
        const std::vector<vx_files::FileSpan> none;
        const vx_files::DirectIo dio(fds, direct);
        vx_files::Readers rd(threads, none, fds, pl, bad.data(), 0, &dio, true);
        vx_merkle::Rounds pack(lens.data(), lens.size(), pl, 0, n, bpr, vx_merkle::Rounds::window_for(bpr, pl),
                               2 * bpr + pl / vx_merkle::kBlock, 4);
        vx_merkle::Round r;
        std::vector<vx_files::ReadItem> items;
        while (pack.next(r)) {
            ++rounds;
            items.clear();
            for (const vx_merkle::Read& x : r.reads) {
                vx_files::ReadItem it{stage + (size_t)x.stage_block * vx_merkle::kBlock, x.piece, 0, x.len};
                it.file = (int32_t)x.file;
                it.file_off = (int64_t)x.file_off;
                items.push_back(it);
            }
            rd.run(items);
            for (const vx_merkle::Read& x : r.reads)
                for (uint64_t at = 0; at < x.len; ++at) {
                    const uint64_t off = x.file_off + at;
                    const uint64_t piece = x.piece + off / pl - x.file_off / pl;
                    if (bad[piece]) continue;
                    mismatches += stage[(size_t)x.stage_block * vx_merkle::kBlock + at] != pattern(x.file, off);
                }
        }
    }
    std::free(raw);
    for (int fd : fds)
        if (fd >= 0) close(fd);
    std::string list;
    for (uint64_t i = 0; i < n; ++i)
        if (bad[i]) list += (list.empty() ? "" : ", ") + std::to_string(i);
    std::printf("{\"pieces\": %llu, \"rounds\": %llu, \"mismatches\": %llu, \"bad\": [%s]}\n", (unsigned long long)n,
                (unsigned long long)rounds, (unsigned long long)mismatches, list.c_str());
    return 0;
}
