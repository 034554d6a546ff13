"""Shapes for the SHA-1 kernels' ring, phase and tile edges, and a model of
which path of a kernel a shape takes.  Host only: no torch, no library (numpy
only in the batches at the end, which carry bytes and states).

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
  chunk_*         the same for the resumable chunk kernel, whose lanes are
                  (length, final); chain_plan: pieces cut into chunks
  *_batch         the long-total lanes and the zero-tail kernels' grid
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


# ---------------------------------------------------------------------------
# The resumable chunk kernel, sha1_ragged_split_kernel<true> (launch_chunk)
# ---------------------------------------------------------------------------
# A lane is (length, final).  A final lane ends its piece: it pads and writes a
# digest.  Any other lane is whole blocks (length % 64 == 0, at least one) and
# stores its state.  Where a lane resumes (poff) and its piece's total length
# do not move an index of the kernel, so they are not part of the shape; the
# GPU sweep assigns them.
def chunk_parts(lane):
    """(nfull, rem, nb) of a lane: nb counts the padding of a final lane only."""
    length, final = lane
    nfull, rem = length >> 6, length & 63
    assert final or (rem == 0 and nfull >= 1), lane
    return nfull, rem, nfull + ((1 if rem <= 55 else 2) if final else 0)


def class_chunk(wave):
    """sha1_ragged_split_kernel<true>: phase 1 trips (0, 1, more), phase 2
    trips (0, 1, 2, more), phase 2 absent (b1 == nb_wave: only a wave without a
    final lane can do that), phase 2 holding no data block, a lane that is not
    final, a final lane with two padding blocks, a lane that is not final and
    ends two blocks or more before the wave does (its state must survive the
    blocks it does not commit), and the block at which the consumer leaves its
    unrolled loop."""
    p = [chunk_parts(x) for x in wave]
    nfull_min, nfull_max = min(x[0] for x in p), max(x[0] for x in p)
    nb_wave = max(x[2] for x in p)
    b1 = nfull_min // kBlockRing * kBlockRing
    p2 = nb_wave - b1
    return (min(b1 // kBlockRing, 2), min(-(-p2 // kBlockRing), 3), p2 == 0, p2 > 0 and nfull_max == b1,
            any(not x[1] for x in wave), any(x[1] and (x[0] & 63) > 55 for x in wave),
            any(not x[1] and nb_wave - y[2] >= 2 for x, y in zip(wave, p)), nb_wave % kAsmUnroll)


def as_final(length):
    return (length, True)


def as_whole_blocks(length):
    """The lane the hybrid path cuts in front of a tail: len & ~63; a piece
    without a whole block becomes one block."""
    return (max(length & ~63, 64), False)


def _odd_lane(wave, k):
    """The lane of a wave that is unlike the rest; of a homogeneous wave, the
    first, a middle or the last lane in turn."""
    if len(set(wave)) == 2:
        return min(range(len(wave)), key=lambda i: wave.count(wave[i]))
    return (0, len(wave) // 2 - 1, len(wave) - 1)[k % 3]


CHUNK_RECIPES = ("final", "whole", "one final", "one whole", "cover")
CHUNK_KINDS = [as_final(64 * f + r) for f in range(64) for r in (0, 55, 56, 63)] + \
    [(64 * f, False) for f in range(1, 64)]


def chunk_waves(recipe):
    """Recipes H and M as chunk waves: every lane final (the GPU sweep resumes
    them all); every lane whole blocks; one final lane among whole-block ones;
    and the reverse.  'cover': see chunk_cover."""
    if recipe == "cover":
        return chunk_cover()
    base = recipe_h() + recipe_m()
    if recipe == "final":
        return [[as_final(L) for L in w] for w in base]
    if recipe == "whole":
        return [[as_whole_blocks(L) for L in w] for w in base]
    many, one = {"one final": (as_whole_blocks, as_final), "one whole": (as_final, as_whole_blocks)}[recipe]
    waves = []
    for k, w in enumerate(base):
        odd = _odd_lane(w, k)
        waves.append([(one if i == odd else many)(L) for i, L in enumerate(w)])
    return waves


def chunk_cover():
    """As recipe_c: for each class of class_chunk that the four recipes above
    leave out, the shortest wave of two kinds of lane that takes it, one odd
    lane among the rest, alternately either kind."""
    if "chunk" not in _cover:
        seen = {class_chunk(w) for r in CHUNK_RECIPES[:-1] for w in chunk_waves(r)}
        kinds = sorted(CHUNK_KINDS)
        spots = (0, WAVE // 2 - 1, WAVE - 1)
        waves = []
        for i, b in enumerate(kinds):
            for a in kinds[:i + 1]:
                c = class_chunk([a, b])
                if c not in seen:
                    seen.add(c)
                    many, one = (a, b) if len(waves) % 2 == 0 else (b, a)
                    w = [many] * WAVE
                    w[spots[len(waves) % 3]] = one
                    waves.append(w)
        _cover["chunk"] = waves
    return _cover["chunk"]


def chunk_batch(recipe):
    """A recipe's lanes in launch order, ending with a wave of one live lane."""
    return flatten(chunk_waves(recipe)) + [as_final(64 * kBlockRing + 57)]


# Block counts of a chain's chunks that are not its last: around the producer's
# ring and the consumer's unrolled loop.
CHAIN_CUTS = sorted({1, kBlockRing - 1, kBlockRing, kBlockRing + 1, 2 * kBlockRing, kAsmUnroll - 1, kAsmUnroll + 1})


def chain_plan():
    """[(length, [chunk bytes, ...])]: one piece per length of GRID that has a
    whole block, cut into one to three chunks of CHAIN_CUTS blocks and the rest.
    The rest is never empty: the kernel takes the chunk that reaches the
    piece's length for its last, so a piece of exactly one block has no cut
    and is left out."""
    rng = random.Random(0xC4A1)
    plan = []
    for L in GRID:
        nfull, cuts, used = L >> 6, [], 0
        if L <= 64:
            continue
        for _ in range(rng.randint(1, 3)):
            fits = [c for c in CHAIN_CUTS if 64 * (used + c) < L]
            if not fits:
                break
            cuts.append(64 * rng.choice(fits))
            used += cuts[-1] >> 6
        plan.append((L, cuts + [L - 64 * used]))
    return plan


# ---------------------------------------------------------------------------
# Batches with their bytes and states (numpy, built once, never modified)
# ---------------------------------------------------------------------------
LONG_TOTALS = (2 ** 29, 2 ** 32 + 64, 2 ** 35)  # 8 * total needs 33, 36 and 39 bits
TAIL_PIECE = 4096
TAIL_LONG_PIECES = (2 ** 29, 2 ** 32)
_batches = {}


def _np():
    import numpy as np

    return np


def chunk_long_batch():
    """Final chunks of 0 to 3 blocks with tails 0, 55, 56 and 63 whose pieces
    are LONG_TOTALS bytes (poff = tlen - len, the incoming states random), 16
    lanes of short totals among them in each wave so that the high word of the
    bit length differs from lane to lane.  The first wave has tlen exactly a
    LONG_TOTAL; the second (63 lanes) tlen = LONG_TOTAL + tail, the totals a
    real piece cut at block boundaries can have.  Fields: buf, offs, lens,
    poffs, tlens (Python ints), states (what the table holds) and start (what
    the kernel must start from: the initial value where poff == 0)."""
    if "chunk_long" not in _batches:
        import types

        import _sha1_model as md

        np = _np()
        shapes = [(f, r) for f in range(4) for r in (0, 55, 56, 63)]
        lanes = []
        for exact in (True, False):
            wave = [(64 * f + r, t if exact else t + r) for t in LONG_TOTALS for f, r in shapes]
            wave += [(64 * f + r, 64 * (k % 3) + 64 * f + r) for k, (f, r) in enumerate(shapes)][:16 if exact else 15]
            random.Random(len(lanes) + 29).shuffle(wave)
            lanes += wave
        lens = np.array([ln for ln, _ in lanes], dtype=np.int64)
        tlens = [t for _, t in lanes]
        poffs = [t - ln for ln, t in lanes]
        offs, size = layout(lens.tolist())
        rng = np.random.default_rng(0x10A6)
        states = rng.integers(0, 2 ** 32, (len(lanes), 5), dtype=np.uint32)
        start = np.where(np.array([p > 0 for p in poffs])[:, None], states, md.IV)
        _batches["chunk_long"] = types.SimpleNamespace(
            buf=rng.integers(0, 256, size + 64, dtype=np.uint8), offs=np.array(offs, dtype=np.int64), lens=lens,
            poffs=poffs, tlens=tlens, states=states, start=start)
    return _batches["chunk_long"]


def _tail_batch(shapes, seed):
    """Lanes (len, pad) with their tail bytes: each tail at a 4-byte aligned
    offset of a buffer that holds 0xFF wherever no tail has a byte, so the
    word that holds a tail's last byte ends in bytes that are not the
    piece's.  Fields: buf, after (the bytes of buf that belong to no tail),
    tail_offs, lens, pads, states (random; garbage where len < 64)."""
    import types

    np = _np()
    lens = np.array([s[0] for s in shapes], dtype=np.int64)
    pads = np.array([s[1] for s in shapes], dtype=np.int64)
    rem = np.where(pads > 0, lens & 63, 0)
    room = (rem + 3) // 4 * 4 + 4
    tail_offs = np.where(rem > 0, 4 + np.cumsum(room) - room, 0)
    rng = np.random.default_rng(seed)
    buf = np.full(int(room.sum()) + 64, 0xFF, dtype=np.uint8)
    after = np.ones(len(buf), dtype=bool)
    for o, r in zip(tail_offs[rem > 0].tolist(), rem[rem > 0].tolist()):
        buf[o:o + r] = rng.integers(0, 256, r, dtype=np.uint8)
        after[o:o + r] = False
    return types.SimpleNamespace(buf=buf, after=after, tail_offs=tail_offs, lens=lens, pads=pads,
                                 states=rng.integers(0, 2 ** 32, (len(shapes), 5), dtype=np.uint32))


def tail_batch():
    """The zero-tail and finish kernels' grid at TAIL_PIECE = 4096: every padded
    length 1..4095 (every rem with every count of zero blocks 0..63, the
    rem == 0 lanes that have no mixed block among them) and one unpadded lane
    to every 16, shuffled, so that a wave mixes all of it; then 64 unpadded
    lanes as one aligned wave of their own.  n % 64 != 0."""
    if "tail" not in _batches:
        shapes = [(L, TAIL_PIECE - L) for L in range(1, TAIL_PIECE)]
        shapes += [(TAIL_PIECE, 0)] * (len(shapes) // 16 + 1)
        random.Random(0x7A11).shuffle(shapes)
        shapes[5 * WAVE:5 * WAVE] = [(TAIL_PIECE, 0)] * WAVE
        if len(shapes) % WAVE == 0:
            shapes.append((TAIL_PIECE, 0))
        _batches["tail"] = _tail_batch(shapes, 0x7A11)
    return _batches["tail"]


def tail_long_batch(piece_length):
    """Padded lanes of a piece_length-byte piece that end 64 * z + (64 - r)
    bytes before it, z zero blocks behind r tail bytes."""
    key = ("tail_long", piece_length)
    if key not in _batches:
        shapes = [(piece_length - 64 * z - (64 - r), 64 * z + 64 - r) for z in (0, 1, 2) for r in (0, 2, 58, 63)]
        _batches[key] = _tail_batch(shapes, piece_length % 1000003)
    return _batches[key]
