"""Shapes for the SHA-1 kernels' ring, phase and tile edges, and a model of
which path of a kernel a shape takes.  Host only: no torch, no library.

Every SHA-1 kernel is an unrolled ring with a remainder path, and which
remainder a piece takes depends on len >> 7, len >> 6 and len & 63 modulo the
ring depths.  The depths are read from the kernel sources, so a change to one
moves the grid, the recipes' coverage check and the GPU sweep with it
(tests/test_sha1_sweep_cpu.py asserts that no class is left out).

  GRID            single lengths: every block count 0..GRID_BLOCKS with every
                  kind of tail (the uniform kernels, and recipe S)
  recipe_*(W)     waves of W lengths: 64 consecutive lanes of a ragged launch,
                  or the 32 pieces of a zero-copy pair
  class_*         pure functions of lengths restating a kernel's index
                  arithmetic: the tuple names the loop trips, the remainder
                  and the branches the shape takes
"""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "vortex_amd", "csrc")


def _constants(path, names):
    with open(path) as f:
        text = f.read()
    out = {}
    for name in names:
        m = re.findall(r"^\s*constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
        if len(m) != 1:
            raise RuntimeError(f"{os.path.basename(path)}: expected one definition of {name}, found {len(m)}; "
                               "the sweep derives its shapes from it")
        out[name] = int(m[0])
    return out


_K = _constants(os.path.join(_CSRC, "vx_kernels.h"), ("kRing", "kLaneRing", "kSplitSlots"))
_K.update(_constants(os.path.join(_CSRC, "sha1_kernels.hip"), ("kBlockRing", "kZcPieces", "kZcTileBlocks")))
kRing, kLaneRing, kSplitSlots = _K["kRing"], _K["kLaneRing"], _K["kSplitSlots"]
kBlockRing, kZcPieces, kZcTileBlocks = _K["kBlockRing"], _K["kZcPieces"], _K["kZcTileBlocks"]


def _asm_unroll():
    """Blocks per trip of the generated consumer (3 LDS slots x 2 word sets)."""
    with open(os.path.join(ROOT, "tools", "gen_sha1_rounds.py")) as f:
        m = re.findall(r"^    for k in range\((\d+)\):  # slots cycle by 3, word sets by 2$", f.read(), re.M)
    if len(m) != 1:
        raise RuntimeError("tools/gen_sha1_rounds.py: the consumer's unroll loop was not found; "
                           "the sweep derives its shapes from it")
    return int(m[0])


kAsmUnroll = _asm_unroll()

WAVE = 64

# Two trips of the widest unrolled loop plus every remainder, in 64-byte
# blocks: the zero-copy kernel takes two tiles per trip, the lane kernels R
# groups of two blocks.
_TRIP = max(2 * kZcTileBlocks, 2 * kLaneRing, 2 * kRing, kBlockRing, kAsmUnroll)
GRID_BLOCKS = 3 * _TRIP
TAILS = (0, 1, 3, 4, 5, 55, 56, 57, 59, 60, 63)
GRID = [64 * f + r for f in range(GRID_BLOCKS + 1) for r in TAILS]


def parts(length):
    """(ng, nfull, rem, nb): 128-byte groups, full 64-byte blocks, tail bytes,
    blocks with the padding."""
    nfull, rem = length >> 6, length & 63
    return nfull >> 1, nfull, rem, nfull + (1 if rem <= 55 else 2)


# ---------------------------------------------------------------------------
# Classifiers
# ---------------------------------------------------------------------------
def class_uniform_lane(length):
    """sha1_uniform_kernel<kLaneRing, false, true>: whole trips of the fenced
    ring (0, 1, more), its remainder, the odd block after it."""
    ng, nfull, _, _ = parts(length)
    return (min(ng // kLaneRing, 2), ng % kLaneRing, nfull & 1)


def class_uniform_split(length, slots=kSplitSlots):
    """sha1_split_kernel<slots>: the producer's ring as for the lane kernel
    (depth kRing), and where the consumer leaves its unrolled loop: block
    nb % 6 of the asm body (slots 3), nb & 1 of the two-slot loop; a second
    padding block or not."""
    ng, nfull, rem, nb = parts(length)
    return (min(ng // kRing, 2), ng % kRing, nfull & 1, nb % kAsmUnroll if slots == 3 else nb & 1, rem > 55)


def class_ragged_lane(wave):
    """sha1_ragged_kernel: trips and remainder of the wave's longest lane, and
    whether a lane runs out of groups before the wave does."""
    ngs = [parts(L)[0] for L in wave]
    ngmax = max(ngs)
    return (min(ngmax // kRing, 2), ngmax % kRing, min(ngs) < ngmax)


def class_ragged_split(wave):
    """sha1_ragged_split_kernel: phase 1 trips, phase 2 trips, phase 2 holding
    only padding, a lane idle for two blocks or more, a lane with two padding
    blocks, a lane with no data block in a wave that runs past both of its
    padding blocks, and the block at which the consumer leaves its loop."""
    p = [parts(L) for L in wave]
    nfull_min = min(x[1] for x in p)
    nb_wave = max(x[3] for x in p)
    b1 = nfull_min // kBlockRing * kBlockRing
    p2 = nb_wave - b1
    return (min(b1 // kBlockRing, 2), min(-(-p2 // kBlockRing), 3), b1 == nfull_min,
            any(nb_wave - x[3] >= 2 for x in p), any(x[2] > 55 for x in p),
            any(x[1] == 0 for x in p) and nb_wave > 2, nb_wave % kAsmUnroll)


def class_zero_copy(wave):
    """sha1_zc_split_kernel: tiles without the select, odd or even number of
    tiles (the trip takes two), blocks in the last tile, and whether the
    consumer's commit is conditional for some block."""
    p = [parts(L) for L in wave]
    b_sel = min(x[1] for x in p)
    nb_wave = max(x[3] for x in p)
    ntiles = -(-nb_wave // kZcTileBlocks)
    return (min(b_sel // kZcTileBlocks, 3), ntiles & 1, nb_wave % kZcTileBlocks, min(x[3] for x in p) == nb_wave)


# ---------------------------------------------------------------------------
# Wave recipes
# ---------------------------------------------------------------------------
H_BLOCKS = range(0, 26)
H_TAILS = (0, 1, 55, 56, 63)
M_SHORT_BLOCKS = (0, 1, 5, 6, 7, 12, 13)
M_EXTRA_BLOCKS = (0, 1, 2, 5, 6, 7, 12, 13)


def recipe_h(width=WAVE):
    """Homogeneous waves: all lanes one length."""
    return [[64 * f + r] * width for f in H_BLOCKS for r in H_TAILS]


def recipe_m(width=WAVE):
    """One lane unlike the rest, both ways round; the odd lane's position
    rotates over the first, a middle and the last lane."""
    spots = (0, width // 2 - 1, width - 1)
    waves = []
    for fs in M_SHORT_BLOCKS:
        for d in M_EXTRA_BLOCKS:
            for rs in (0, 56):
                for rl in (55, 63):
                    short, long_ = 64 * fs + rs, 64 * (fs + d) + rl
                    for many, one in ((short, long_), (long_, short)):
                        w = [many] * width
                        w[spots[len(waves) % 3]] = one
                        waves.append(w)
    return waves


def wave_classifiers(width=WAVE):
    return (class_ragged_lane, class_ragged_split) if width == WAVE else (class_zero_copy,)


_cover = {}


def recipe_c(width=WAVE):
    """Cover: H and M reach every combination of phase 1 and phase 2 trips, but
    not every class of the wave classifiers (M's block counts leave out some
    values of nb_wave % 6 beside each of them, and never reach three tiles
    without the select).  For each class they leave out, the smallest wave of
    two lengths that takes it, one odd lane among the rest, alternately the
    long one and the short one."""
    if width not in _cover:
        fns = wave_classifiers(width)
        seen = [{fn(w) for w in recipe_h(width) + recipe_m(width)} for fn in fns]
        lengths = [64 * f + r for f in range(GRID_BLOCKS + 1) for r in (0, 55, 56, 63)]
        spots = (0, width // 2 - 1, width - 1)
        waves = []
        for i, long_ in enumerate(lengths):
            for short in lengths[:i + 1]:
                new = False
                for fn, have in zip(fns, seen):
                    c = fn([short, long_])
                    if c not in have:
                        have.add(c)
                        new = True
                if new:
                    many, one = (short, long_) if len(waves) % 2 == 0 else (long_, short)
                    w = [many] * width
                    w[spots[len(waves) % 3]] = one
                    waves.append(w)
        _cover[width] = waves
    return _cover[width]


def flatten(waves):
    return [L for w in waves for L in w]


def batch_waves(width=WAVE):
    """Recipes H, M and C as one batch, ending (T) with a wave of one live lane."""
    return flatten(recipe_h(width) + recipe_m(width) + recipe_c(width)) + [64 * kBlockRing + 57]


def batch_s():
    """GRID shuffled with a fixed seed (its last wave is partial too)."""
    lens = list(GRID)
    random.Random(0x5EED).shuffle(lens)
    return lens


def waves_of(lens, width=WAVE):
    """The waves of a launch over `lens` in lane order: the dead lanes of a
    partial last wave repeat the last piece, so they add no length."""
    return [lens[i:i + width] for i in range(0, len(lens), width)]


def layout(lens, gap=16):
    """16-byte aligned offsets with a gap after each piece, and the size."""
    offs, o = [], 16
    for L in lens:
        offs.append(o)
        o += (L + 15) // 16 * 16 + gap
    return offs, o
