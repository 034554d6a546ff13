// vx_merkle_tree.hpp — the host side of the layer trees (vx_hash.h, "Layer
// trees"): the planner of vx_merkle_device_trees, the layout of
// a torrent's trees and the proof lookup.  Host only, no HIP.
//
// The tree of a layer of m rows keeps every level k = 0..K = ceil(log2 m), level
// k holding n_k = ceil(m / 2^k) rows, back to back with level 0 first.  The pass
// rule is plan_layers' (vx_merkle_layers.hpp): a layer whose level 9p holds m_p
// rows is one tile of ceil(log2 m_p) levels when m_p <= 512 and ceil(m_p / 512)
// tiles of 9 levels otherwise.  Where the layers planner sends a tile's top to a
// work area, a tree tile stores every level it reduces at that level's place in
// the tree, so its top lands in level 9(p + 1), which is what pass p + 1 reads.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "vx_merkle_layers.hpp"

namespace vx_merkle {

static_assert(sizeof(vx_merkle_tree_tile) == 16 && sizeof(struct vx_merkle_tree_plan) == 48, "the ABI's layouts");

// Rows of the tree of an m-row layer: sum of ceil(m / 2^k), k = 0..ceil(log2 m).
inline uint64_t tree_rows(uint64_t m) {
    if (m == 0) return 0;
    uint64_t rows = m;
    while (m > 1) {
        m = (m + 1) >> 1;
        rows += m;
    }
    return rows;
}

// First row of level `level` in the tree of an m-row layer (level <= K + 1).
inline uint64_t level_off(uint64_t m, uint32_t level) {
    uint64_t off = 0;
    for (uint32_t k = 0; k < level; ++k) {
        off += m;
        m = (m + 1) >> 1;
    }
    return off;
}

// One walk over the passes: counts the tiles (tiles == NULL) or writes them, as
// walk_layers does.  tree_off (may be NULL) gets n_layers + 1 row offsets.
// VX_EINVAL: a count of 0, or 2^32 or more rows in the layers, in the trees
// (the descriptors hold rows as 32-bit numbers) or in the tiles.
inline int walk_trees(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_tree_plan* plan,
                      vx_merkle_tree_tile* tiles, uint64_t* tree_off) {
    uint64_t rows = 0, trows = 0;
    for (uint32_t f = 0; f < n_layers; ++f) {
        if (counts[f] == 0) return VX_EINVAL;
        rows += counts[f];
        trows += tree_rows(counts[f]);
    }
    if ((rows >> 32) || (trows >> 32)) return VX_EINVAL;
    struct vx_merkle_tree_plan pl = {};
    pl.n_layers = n_layers;
    pl.rows = rows;
    pl.tree_rows = trows;
    uint64_t n_tiles = 0;
    for (uint32_t p = 0; p < 4; ++p) {
        uint64_t in = 0, off = 0, pass_tiles = 0;  // layer f's first row in d_hashes / in the tree buffer
        for (uint32_t f = 0; f < n_layers; ++f) {
            const uint64_t in_f = in, off_f = off;
            in += counts[f];
            off += tree_rows(counts[f]);
            // rows of layer f at level 9p: counts[f] divided by 512 p times, rounding up each time
            uint64_t m = counts[f];
            bool alive = true;
            for (uint32_t q = 0; q < p && alive; ++q) {
                alive = m > kTileRows;
                m = (m + kTileRows - 1) >> kTileLevels;
            }
            if (!alive) continue;
            const uint64_t nt = (m + kTileRows - 1) >> kTileLevels;
            if (tiles) {
                const uint64_t dst = off_f + level_off(counts[f], kTileLevels * p);
                for (uint64_t k = 0; k < nt; ++k) {
                    vx_merkle_tree_tile t = {};
                    t.src_row = (uint32_t)(p == 0 ? in_f : dst);
                    t.dst_row = (uint32_t)dst;
                    t.level_rows = (uint32_t)m;
                    t.tile = (uint32_t)k;
                    tiles[n_tiles + pass_tiles + k] = t;
                }
            }
            pass_tiles += nt;
        }
        if (pass_tiles == 0) break;
        if ((n_tiles + pass_tiles) >> 32) return VX_EINVAL;
        pl.pass_tiles[p] = (uint32_t)pass_tiles;
        pl.passes = p + 1;
        n_tiles += pass_tiles;
    }
    pl.n_tiles = (uint32_t)n_tiles;
    *plan = pl;
    if (tree_off) {
        uint64_t off = 0;
        for (uint32_t f = 0; f < n_layers; ++f) {
            tree_off[f] = off;
            off += tree_rows(counts[f]);
        }
        tree_off[n_layers] = off;
    }
    return 0;
}

// vx_merkle_tree_plan without its error text.  With tiles given and tiles_cap <
// n_tiles nothing is written to tiles or tree_off (the count comes first).
inline int plan_trees(const uint32_t* counts, uint32_t n_layers, struct vx_merkle_tree_plan* plan,
                      vx_merkle_tree_tile* tiles, size_t tiles_cap, uint64_t* tree_off) {
    if (!plan || (n_layers && !counts)) return VX_EINVAL;
    int rc = walk_trees(counts, n_layers, plan, nullptr, tiles ? nullptr : tree_off);
    if (rc || !tiles) return rc;
    if (tiles_cap < plan->n_tiles) return VX_EINVAL;
    return walk_trees(counts, n_layers, plan, tiles, tree_off);
}

// vx_merkle_tree_layout: per file the rows of its layer (0: an empty file, 1: a
// file of at most piece_length bytes, its `pieces root`) and where its tree
// starts.  Returns the total rows, or -1 when a file has 2^32 or more pieces.
inline int64_t tree_layout(const uint64_t* file_lengths, size_t nfiles, uint32_t piece_length, uint32_t* counts_out,
                           uint64_t* tree_off_out) {
    uint64_t off = 0;
    for (size_t f = 0; f < nfiles; ++f) {
        const uint64_t m = (file_lengths[f] + piece_length - 1) / piece_length;
        if (m >> 32) return -1;
        if (counts_out) counts_out[f] = (uint32_t)m;
        if (tree_off_out) tree_off_out[f] = off;
        off += tree_rows(m);
    }
    if (tree_off_out) tree_off_out[nfiles] = off;
    return (int64_t)off;
}

// pads: pad(h) for h = 0..kProofPads - 1, 32 bytes each (the caller's table:
// this header hashes nothing).  height + level + 9 + 64 fits: height <= 64 and
// level <= 32.
constexpr uint32_t kProofPads = 64 + 32 + 9 + 64 + 1;

// vx_merkle_tree_proof over a table of pad hashes.  Row j of level k of the
// tree, or pad(height + k) where the tree stores none.  VX_EINVAL as the entry
// documents it.
inline int tree_proof(const uint8_t* tree, uint32_t m, uint32_t height, uint32_t level, uint64_t pos, uint32_t span,
                      uint32_t uncles, const uint8_t* pads, uint8_t* out) {
    if (!tree || !out || !pads || m == 0 || height > 64) return VX_EINVAL;
    if (span == 0 || span > kTileRows || (span & (span - 1)) || uncles > 64) return VX_EINVAL;
    const uint32_t K = ceil_log2(m);
    if (level > K) return VX_EINVAL;
    const uint64_t n_level = ((uint64_t)m + (1ull << level) - 1) >> level;
    if (pos >= (n_level + span - 1) / span) return VX_EINVAL;  // the span holds no row of the level
    auto row = [&](uint32_t k, uint64_t j, uint8_t* dst) {
        const uint64_t n_k = k > K ? 0 : ((uint64_t)m + (1ull << k) - 1) >> k;
        if (j < n_k)
            memcpy(dst, tree + (level_off(m, k) + j) * 32, 32);
        else
            memcpy(dst, pads + (size_t)(height + k) * 32, 32);
    };
    for (uint32_t k = 0; k < span; ++k) row(level, pos * span + k, out + (size_t)k * 32);
    const uint32_t base = level + ceil_log2(span);
    for (uint32_t t = 0; t < uncles; ++t) {
        // (past 63 steps pos has no bits left: the running node is node 0, its sibling node 1)
        const uint64_t j = (t < 64 ? pos >> t : 0) ^ 1;
        // node 0 of a level above K is a hash of real rows that the tree does not store;
        // pos < ceil(n_level / span) keeps j at 1 there
        row(base + t, j, out + (size_t)(span + t) * 32);
    }
    return 0;
}

}  // namespace vx_merkle
