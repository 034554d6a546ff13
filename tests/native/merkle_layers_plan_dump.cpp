// merkle_layers_plan_dump — the planner of vx_merkle_device_layers
// (vortex_amd/csrc/vx_merkle_layers.hpp) as a stand-alone program, so the test
// can run it under ASan+UBSan without a GPU (tests/test_merkle_layers_cpu.py).
//
//   merkle_layers_plan_dump dump     counts on stdin, one per line; prints
//       "T pass in_row out rows levels last" per tile, then the plan as JSON.
//       The tile array is exactly n_tiles long (heap), so a tile written past
//       it is an ASan error.
//   merkle_layers_plan_dump errors   counts on stdin (a valid list); checks
//       what the planner refuses and that a refused call leaves the tile array
//       and a guard region behind it untouched; prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vx_merkle_layers.hpp"

static int die(const char* what) {
    std::fprintf(stderr, "merkle_layers_plan_dump: %s\n", what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 2) return die("usage: merkle_layers_plan_dump dump|errors < counts");
    std::vector<uint32_t> counts;
    unsigned long long v;
    while (std::scanf("%llu", &v) == 1) counts.push_back((uint32_t)v);
    const uint32_t n = (uint32_t)counts.size();
    struct vx_merkle_layers_plan plan;
    if (!std::strcmp(argv[1], "dump")) {
        if (vx_merkle::plan_layers(counts.data(), n, &plan, nullptr, 0)) return die("the counts were refused");
        vx_merkle_tile* tiles = static_cast<vx_merkle_tile*>(std::malloc(sizeof(vx_merkle_tile) * (plan.n_tiles + !plan.n_tiles)));
        struct vx_merkle_layers_plan again;
        if (vx_merkle::plan_layers(counts.data(), n, &again, tiles, plan.n_tiles)) return die("refused with tiles");
        if (std::memcmp(&plan, &again, sizeof plan)) return die("the plan differs between the two calls");
        uint32_t t = 0;
        for (uint32_t p = 0; p < plan.passes; ++p)
            for (uint32_t k = 0; k < plan.pass_tiles[p]; ++k, ++t)
                std::printf("T %u %u %u %u %u %u\n", p, tiles[t].in_row, tiles[t].out, (unsigned)tiles[t].rows,
                            (unsigned)tiles[t].levels, (unsigned)tiles[t].last);
        std::printf("{\"n_layers\": %u, \"passes\": %u, \"rows\": %llu, \"work_rows\": %llu, \"n_tiles\": %u, "
                    "\"pass_tiles\": [%u, %u, %u, %u]}\n",
                    plan.n_layers, plan.passes, (unsigned long long)plan.rows, (unsigned long long)plan.work_rows,
                    plan.n_tiles, plan.pass_tiles[0], plan.pass_tiles[1], plan.pass_tiles[2], plan.pass_tiles[3]);
        std::free(tiles);
        return 0;
    }
    if (std::strcmp(argv[1], "errors")) return die("unknown mode");
    if (n < 2 || vx_merkle::plan_layers(counts.data(), n, &plan, nullptr, 0) || plan.n_tiles < 2)
        return die("errors needs a valid list of at least two counts");
    // tiles_cap = n_tiles - 1: refused, and neither the array nor the guard behind it is touched
    const size_t guard = 64, cap = plan.n_tiles - 1;
    std::vector<uint8_t> buf((cap + guard) * sizeof(vx_merkle_tile), 0xA5);
    struct vx_merkle_layers_plan out;
    if (vx_merkle::plan_layers(counts.data(), n, &out, reinterpret_cast<vx_merkle_tile*>(buf.data()), cap) != VX_EINVAL)
        return die("tiles_cap = n_tiles - 1 was accepted");
    for (uint8_t b : buf)
        if (b != 0xA5) return die("a refused call wrote to tiles");
    // ... and with tiles_cap = n_tiles the guard stays as it was
    if (vx_merkle::plan_layers(counts.data(), n, &out, reinterpret_cast<vx_merkle_tile*>(buf.data()), cap + 1))
        return die("tiles_cap = n_tiles was refused");
    for (size_t k = (cap + 1) * sizeof(vx_merkle_tile); k < buf.size(); ++k)
        if (buf[k] != 0xA5) return die("the planner wrote past n_tiles");
    // a zero count, anywhere
    for (uint32_t at : {0u, n / 2, n - 1}) {
        std::vector<uint32_t> c = counts;
        c[at] = 0;
        if (vx_merkle::plan_layers(c.data(), n, &out, nullptr, 0) != VX_EINVAL) return die("a zero count was accepted");
    }
    // a sum of exactly 2^32 is refused, 2^32 - 1 is planned (tiles == NULL: nothing to allocate)
    const uint32_t half[2] = {0x80000000u, 0x80000000u}, most[2] = {0x80000000u, 0x7FFFFFFFu};
    if (vx_merkle::plan_layers(half, 2, &out, nullptr, 0) != VX_EINVAL) return die("a sum of 2^32 was accepted");
    if (vx_merkle::plan_layers(most, 2, &out, nullptr, 0)) return die("a sum of 2^32 - 1 was refused");
    if (out.rows != 0xFFFFFFFFull || out.passes != 4 || out.pass_tiles[0] != (1u << 22) + (1u << 22) ||
        out.pass_tiles[3] != 2 || out.n_tiles != out.pass_tiles[0] + out.pass_tiles[1] + out.pass_tiles[2] + 2)
        return die("the plan of 2^31 + (2^31 - 1) rows is wrong");
    const uint32_t one = 0xFFFFFFFFu;
    if (vx_merkle::plan_layers(&one, 1, &out, nullptr, 0) || out.passes != 4 || out.pass_tiles[3] != 1)
        return die("one layer of 2^32 - 1 rows must take four passes");
    // no layers: an empty plan
    if (vx_merkle::plan_layers(nullptr, 0, &out, nullptr, 0) || out.passes || out.n_tiles || out.rows || out.work_rows)
        return die("no layers must give an empty plan");
    if (vx_merkle::plan_layers(counts.data(), n, nullptr, nullptr, 0) != VX_EINVAL) return die("a NULL plan was accepted");
    std::puts("ok");
    return 0;
}
