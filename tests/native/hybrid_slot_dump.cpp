// hybrid_slot_dump — vortex_amd/csrc/vx_hybrid_slot.hpp as a stand-alone
// program (tests/test_hybrid_async_cpu.py builds it with ASan + UBSan and
// compares every line with a Python model).  Reads lines from stdin:
//   L max_piece_len off len pad log2w flags
//       -> "L rc chunk total tail_off zero_blocks mixed flags" (after a
//          rejection: "L rc" only, the reason on stderr)
//   P n -> "P" and the offsets of vx_hybrid_slot::pack(n), in struct order
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "vx_hybrid_slot.hpp"

int main() {
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'L') {
            uint64_t off = 0;
            uint32_t mpl = 0, len = 0, pad = 0, log2w = 0, flags = 0;
            if (std::sscanf(line + 1, "%" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &mpl, &off,
                            &len, &pad, &log2w, &flags) != 6)
                return 2;
            const char* why = nullptr;
            const int rc = vx_hybrid_slot::check(len, pad, log2w, mpl, &why);
            if (rc) {
                std::fprintf(stderr, "%u %u %u: %s\n", len, pad, log2w, why);
                std::printf("L %d\n", rc);
                continue;
            }
            const vx_hybrid_slot::Lane l = vx_hybrid_slot::lane(off, len, pad, (uint8_t)flags);
            std::printf("L 0 %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu32 " %d %d\n", l.chunk, l.total, l.tail_off,
                        l.zero_blocks, (int)l.mixed, (int)l.flags);
        } else if (line[0] == 'P') {
            uint32_t n = 0;
            if (std::sscanf(line + 1, "%" SCNu32, &n) != 1) return 2;
            const vx_hybrid_slot::Pack p = vx_hybrid_slot::pack(n);
            std::printf("P %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", p.offsets,
                        p.tail_offs, p.totals, p.poffs, p.src, p.lens, p.pads, p.chunks, p.ident, p.rows, p.tfirst,
                        p.exp_sha1, p.exp_roots, p.flags, p.log2w, p.copy_bytes, p.states, p.bytes);
        } else if (line[0] != '\n') {
            return 2;
        }
    }
    return 0;
}
