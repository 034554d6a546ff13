// vx_merkle_layers.hpp — the planner of vx_merkle_device_layers (vx_hash.h,
// "Segmented layer roots").  Host only, no HIP: the layer sizes
// follow from the file lengths, so the host cuts every layer into tiles of one
// workgroup each and the device only executes them, pass after pass.
//
// The pass rule is launch_merkle_root's, applied per layer: a layer of m rows
// alive at pass p is one last tile of ceil(log2 m) levels when m <= 512, and
// ceil(m / 512) tiles of 9 levels otherwise, whose tops (consecutive rows of
// the work area, never reused) are the layer at pass p + 1.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "vx_hash.h"

namespace vx_merkle {

constexpr uint32_t kTileRows = VX_MERKLE_TILE_ROWS;
constexpr uint32_t kTileLevels = 9;
static_assert(kTileRows == 1u << kTileLevels, "a tile reduces 9 levels");
static_assert(sizeof(vx_merkle_tile) == 16 && sizeof(vx_merkle_proof) == 24 &&
                  sizeof(struct vx_merkle_layers_plan) == 48,
              "the ABI's layouts");

inline uint32_t ceil_log2(uint32_t m) {
    uint32_t l = 0;
    while ((1ull << l) < m) ++l;
    return l;
}

// One walk over the passes: counts the tiles (emit == false) or writes them.
// The state of a layer between passes is (first input row, rows); it is
// recomputed from counts[] in each pass instead of being stored, so the planner
// allocates nothing: pass p's work rows start where pass p - 1's ended.
// Returns VX_EINVAL for a count of 0, a sum of counts >= 2^32 or more than
// 2^32 - 1 tiles.
inline int walk_layers(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_layers_plan* plan,
                       vx_merkle_tile* tiles) {
    uint64_t rows = 0;
    for (uint32_t f = 0; f < n_layers; ++f) {
        if (counts[f] == 0) return VX_EINVAL;
        rows += counts[f];
    }
    if (rows >> 32) return VX_EINVAL;
    struct vx_merkle_layers_plan pl = {};
    pl.n_layers = n_layers;
    pl.rows = rows;
    uint64_t n_tiles = 0;
    uint64_t work_lo = 0, work_hi = 0;  // the rows pass p reads / the rows written so far
    for (uint32_t p = 0; p < 4; ++p) {
        uint64_t in = p == 0 ? 0 : work_lo;  // first input row of the next alive layer
        uint64_t out = work_hi, pass_tiles = 0;
        for (uint32_t f = 0; f < n_layers; ++f) {
            // rows of layer f at pass p: counts[f] divided by 512 p times, rounding up each time
            uint64_t m = counts[f];
            bool alive = true;
            for (uint32_t q = 0; q < p && alive; ++q) {
                alive = m > kTileRows;
                m = (m + kTileRows - 1) >> kTileLevels;
            }
            if (!alive) continue;
            if (m <= kTileRows) {
                if (tiles) {
                    vx_merkle_tile t = {};
                    t.in_row = (uint32_t)in;
                    t.out = f;
                    t.rows = (uint16_t)m;
                    t.levels = (uint8_t)ceil_log2((uint32_t)m);
                    t.last = 1;
                    tiles[n_tiles + pass_tiles] = t;
                }
                ++pass_tiles;
            } else {
                const uint64_t nt = (m + kTileRows - 1) >> kTileLevels;
                if (tiles) {
                    for (uint64_t k = 0; k < nt; ++k) {
                        vx_merkle_tile t = {};
                        t.in_row = (uint32_t)(in + k * kTileRows);
                        t.out = (uint32_t)(out + k);
                        const uint64_t left = m - k * kTileRows;
                        t.rows = (uint16_t)(left < kTileRows ? left : kTileRows);
                        t.levels = (uint8_t)kTileLevels;
                        t.last = 0;
                        tiles[n_tiles + pass_tiles + k] = t;
                    }
                }
                pass_tiles += nt;
                out += nt;
            }
            in += m;
        }
        if (pass_tiles == 0) break;
        if ((n_tiles + pass_tiles) >> 32) return VX_EINVAL;
        pl.pass_tiles[p] = (uint32_t)pass_tiles;
        pl.passes = p + 1;
        n_tiles += pass_tiles;
        work_lo = work_hi;
        work_hi = out;
    }
    pl.n_tiles = (uint32_t)n_tiles;
    pl.work_rows = work_hi;
    *plan = pl;
    return 0;
}

// vx_merkle_layers_plan without its error text.  With tiles given and
// tiles_cap < n_tiles nothing is written to tiles (the count comes first).
inline int plan_layers(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_layers_plan* plan,
                       vx_merkle_tile* tiles, size_t tiles_cap) {
    if (!plan || (n_layers && !counts)) return VX_EINVAL;
    int rc = walk_layers(counts, n_layers, plan, nullptr);
    if (rc || !tiles) return rc;
    if (tiles_cap < plan->n_tiles) return VX_EINVAL;
    return walk_layers(counts, n_layers, plan, tiles);
}

}  // namespace vx_merkle
