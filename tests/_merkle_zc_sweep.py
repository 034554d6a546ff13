"""Shapes for merkle_zc_piece_kernel (sha256_kernels.hip; vx_set_merkle_zero_copy)
on its own, the hashlib model of its results and a classifier of which path a
lane, a wave and a launch take.  Host only: no torch; numpy for the bytes.

The kernel's leaf phase, restated: thread i of a workgroup owns leaf row i of
the workgroup's GEO.group rows; a wave serves GEO.wave leaves.  A leaf of
leaf_len bytes is nt = leaf_len // T full tiles (T = GEO.tile bytes), loaded
cooperatively by the wave and run to the wave's largest count nt_wave with
GEO.inflight register tiles in turn, then rem = leaf_len % T bytes through the
owning lane's finish_tail (the constant padding block for a full leaf, the zero
row for a slot at or past the piece's end).  The tree phase and the tops
protocol are merkle_piece_kernel's.

  geometry()           the four numbers of vx_tuning_merkle_zc_geometry, and lds_bytes()
  lengths(geo, W)      the single piece lengths of the issue's list, for a tree of W leaves
  launches(geo)        [Launch]: every launch of the sweep, built from the geometry
  classes(geo, launch) the set of classes one launch reaches
  REQUIRED             every class the sweep has to reach
  place(launch)        the bytes: (buffer filled with FILL, [source offset per piece])
  model(launch, buf, offs)
                       hashlib roots, and the expected rows and verdicts of a launch
"""
import collections
import ctypes
import random

import numpy as np

LEAF = 16384
FILL = 0xA5
SEED = 0x2C5EED

Geo = collections.namedtuple("Geo", "group wave tile inflight")
# pieces: [(length, log2w)]; K: the launch's log2_width; expect: "rows" (correct / first word off / last word
# off by piece index mod 3) or "null" (roots only)
Launch = collections.namedtuple("Launch", "name K pieces expect")


def geometry():
    from vortex_amd import _lib

    out = (ctypes.c_uint32 * 4)()
    _lib.tuning().vx_tuning_merkle_zc_geometry(out)
    return Geo(*out)


def lds_bytes(geo):
    """A stage of tile / 16 rows of wave + 1 16-byte slots per wave, and the workgroup's 32-byte leaf rows."""
    return (geo.group // geo.wave) * (geo.tile // 16) * (geo.wave + 1) * 16 + geo.group * 32


def lengths(geo, W):
    """The issue's single lengths for a piece whose own tree has W leaves (those that fit it)."""
    T, F = geo.tile, geo.inflight
    odd = 3 if F % 2 == 0 else 1  # an odd and an even number of tiles, a multiple of the tiles in flight and one more
    want = [0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1,
            odd * T, 4 * T, 2 * F * T, 2 * F * T + T, 2 * F * T + T + 9, 16383, 16384, 16385, W * LEAF - 1, W * LEAF]
    return [v for v in dict.fromkeys(want) if v <= W * LEAF]


def _wave_recipes(geo):
    """{name: geo.wave leaf lengths}: one wave each, at width 0 (a piece is a leaf)."""
    rng = random.Random(SEED)
    w, T = geo.wave, geo.tile
    step = LEAF // (w - 1)
    F = geo.inflight
    return {
        # the wave's largest tile count a multiple of the tiles in flight, and one more than that
        "inflight_multiple": [2 * F * T] + [rng.randrange(2 * F * T) for _ in range(w - 1)],
        "inflight_plus_one": [rng.randrange(2 * F * T) for _ in range(w - 1)] + [2 * F * T + T + 9],
        "all_full": [LEAF] * w,
        "tails_only": [1 + rng.randrange(T - 1) for _ in range(w)],
        "mixed": [rng.choice([0, 1, T - 1, T, 3 * T + 5, LEAF - 1, LEAF, rng.randrange(LEAF + 1)]) for _ in range(w)],
        "ascending": [min(LEAF, k * step + (k % 3)) for k in range(w)],
        "descending": [min(LEAF, (w - 1 - k) * step + (k % 5)) for k in range(w)],
    }


def launches(geo):
    rng = random.Random(SEED + 1)
    out = []
    # every single length, at the piece's own width 1 or 0 in a launch of width 1; with rows and without
    singles = [(v, 1 if v > LEAF or k % 2 else 0) for k, v in enumerate(lengths(geo, 2))]
    out.append(Launch("lengths", 1, singles, "rows"))
    out.append(Launch("lengths_no_rows", 1, singles, "null"))
    # the wave recipes, one wave each, in one launch of width 0
    waves = [(v, 0) for lens in _wave_recipes(geo).values() for v in lens]
    out.append(Launch("waves", 0, waves, "rows"))
    # whole waves of slots past the pieces' ends: width log2(wave), pieces of 0 bytes and of one leaf and a bit
    kw = geo.wave.bit_length() - 1
    out.append(Launch("past_end", kw, [(0, kw), (LEAF + 5, kw), (3, kw), (0, kw)], "rows"))
    # every width 0..8 in a launch of its own: one more piece than a workgroup holds, own widths 0..K
    for K in range(9):
        per = geo.group >> K
        pieces = []
        for i in range(per + 1):
            lw = (i + K) % (K + 1)
            cap = LEAF << lw
            v = (cap, cap - 1, 0, rng.randrange(cap + 1), min(cap, 2 * geo.tile + 1), min(cap, LEAF + 1))[i % 6]
            if K >= 6 and i % 6 in (0, 1) and i >= 2:
                v = rng.randrange(2 * LEAF)  # (few long pieces in the widest launches)
            pieces.append((v, lw))
        out.append(Launch(f"width{K}", K, pieces, "rows"))
    # piece counts around a workgroup's, and one piece
    for K in (0, 3, 6):
        per = geo.group >> K
        for n in sorted({per - 1, per, per + 1, 1}):
            if n:
                out.append(Launch(f"count{K}_{n}", K, [(rng.randrange(min(LEAF << K, 3 * LEAF) + 1), K)
                                                       for _ in range(n)], "rows"))
    # the tops path: widths 9 and 10, one and three pieces, own widths at, below and far below the launch's
    for K in (9, 10):
        W = 1 << K
        out.append(Launch(f"tops{K}_1", K, [(W * LEAF, K)], "rows"))
        out.append(Launch(f"tops{K}_3", K, [(W * LEAF - 1, K), ((W // 2) * LEAF, K - 1), (5 * LEAF + 77, 3)], "rows"))
    return out


def leaf_lens(launch):
    """Leaf length of every lane of the launch's grid rows (n << K), row-major."""
    W = 1 << launch.K
    return [max(0, min(LEAF, v - s * LEAF)) for v, _ in launch.pieces for s in range(W)]


def classes(geo, launch):
    got = set()
    K, n = launch.K, len(launch.pieces)
    T, F, w = geo.tile, geo.inflight, geo.wave
    per = max(1, geo.group >> K)
    got.add("tops" if K > 8 else "narrow")
    got.add(f"K{K}")
    if any(lw < K for _, lw in launch.pieces):
        got.add("log2w_below")
    if (n << K) > geo.group:
        got.add("multi_workgroup")
    if K <= 8:
        got |= {c for c, hit in (("n1", n == 1), ("n_per_minus1", n == per - 1), ("n_per", n == per),
                                 ("n_per_plus1", n == per + 1)) if hit}
    if K > 8:
        got.add(f"tops_n{n}")
    got.add("expect_" + launch.expect)
    for v, lw in launch.pieces:
        if v == 0:
            got.add("zero_piece")
        if v == (LEAF << lw):
            got.add("len_W_leaves")
        if v == (LEAF << lw) - 1:
            got.add("len_W_leaves_minus1")
    lens = leaf_lens(launch)
    lens += [0] * (-len(lens) % geo.group)  # lanes past the launch's rows hash nothing
    if len(lens) != (n << K):
        got.add("lanes_past_rows")
    for ll in lens:
        nt, rem = divmod(ll, T)
        if ll == LEAF:
            got.add("leaf_full")
        elif ll == 0:
            got.add("leaf_empty")
        elif nt == 0:
            got.add("leaf_tail_only")
        else:
            got.add("leaf_tiles_then_tail" if rem else "leaf_tiles_exact")
        if 0 < ll < LEAF:
            got.add("pad_in_block" if rem % 64 <= 55 else "pad_next_block")
            if rem % 4:
                got.add("tail_partial_word")
    for k in range(0, len(lens), w):
        wave = lens[k:k + w]
        nts = [ll // T for ll in wave]
        m = max(nts)
        if all(ll == 0 for ll in wave):
            got.add("wave_idle")
        elif m == 0:
            got.add("wave_tails_only")
        elif all(ll == LEAF for ll in wave):
            got.add("wave_all_full")
        elif len(set(nts)) > 1:
            got.add("wave_mixed")
        if m:
            got.add("wave_odd_tiles" if m % 2 else "wave_even_tiles")
            got.add({0: "wave_inflight_multiple", 1: "wave_inflight_plus_one"}.get(m % F, "wave_inflight_other"))
        if len(set(wave)) > w // 2:
            if all(a <= b for a, b in zip(nts, nts[1:])):
                got.add("wave_ascending")
            if all(a >= b for a, b in zip(nts, nts[1:])):
                got.add("wave_descending")
    return got


REQUIRED = ({"narrow", "tops", "log2w_below", "multi_workgroup", "n1", "n_per_minus1", "n_per", "n_per_plus1",
             "tops_n1", "tops_n3", "expect_rows", "expect_null", "zero_piece", "len_W_leaves", "len_W_leaves_minus1",
             "lanes_past_rows", "leaf_full", "leaf_empty", "leaf_tail_only", "leaf_tiles_then_tail",
             "leaf_tiles_exact", "pad_in_block", "pad_next_block", "tail_partial_word", "wave_idle",
             "wave_tails_only", "wave_all_full", "wave_mixed", "wave_odd_tiles", "wave_even_tiles",
             "wave_inflight_multiple", "wave_inflight_plus_one", "wave_ascending", "wave_descending"}
            | {f"K{K}" for K in range(11)})


def place(launch, seed=0):
    """The launch's bytes: one buffer filled with FILL, the pieces' random bytes at 16-byte aligned offsets
    that are no multiple of 256, with a gap behind every piece, laid out in a shuffled order (so the sources
    are not in address order).  Returns (numpy buffer, [offset per piece])."""
    rng = random.Random(SEED + 2 + seed)
    order = list(range(len(launch.pieces)))
    rng.shuffle(order)
    offs, cur = [0] * len(order), 0
    for i in order:
        cur = (cur + 15) // 16 * 16 + 16 * (1 + rng.randrange(15))
        if cur % 256 == 0:
            cur += 16
        offs[i] = cur
        cur += launch.pieces[i][0]
    buf = np.full(cur + 4096, FILL, dtype=np.uint8)
    data = np.random.default_rng(SEED + seed).integers(0, 256, cur, dtype=np.uint8)
    for i, (v, _) in enumerate(launch.pieces):
        buf[offs[i]:offs[i] + v] = data[offs[i]:offs[i] + v]
    return buf, offs


def source_classes(offs, pieces):
    got = set()
    if any(a > b for a, b in zip(offs, offs[1:])):
        got.add("unordered")
    if all(o % 16 == 0 for o in offs) and any(o % 256 for o in offs):
        got.add("aligned16_not256")
    ends = sorted((o, o + v) for o, (v, _) in zip(offs, pieces))
    if all(b[0] - a[1] >= 1 for a, b in zip(ends, ends[1:])):
        got.add("gaps")
    return got


def model(launch, buf, offs):
    """(roots, expected rows or None, verdicts or None): hashlib over the pieces' own bytes."""
    from vortex_amd import hybrid

    raw = buf.tobytes()
    roots = [hybrid.v2_root(raw[o:o + v], lw) for o, (v, lw) in zip(offs, launch.pieces)]
    if launch.expect == "null":
        return roots, None, None
    rows, verdicts = [], []
    for i, r in enumerate(roots):
        row = bytearray(r)
        if i % 3 == 1:
            row[3] ^= 0x10   # one bit off in the first word
        elif i % 3 == 2:
            row[31] ^= 0x01  # one bit off in the last word
        rows.append(bytes(row))
        verdicts.append(1 if i % 3 == 0 else 0)
    return roots, rows, verdicts
