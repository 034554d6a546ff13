"""Shapes for the SHA-256 leaf lanes and tree reductions of sha256_kernels.hip
on their own, the BEP 52 model of their results and a classifier of which path
a lane or a piece takes.  Host only: no torch, no library; numpy for the bytes.

The leaf lane (merkle_leaf_kernel<true> and <false>, merkle_block_check_kernel,
merkle_block_kernel, merkle_piece_kernel): leaf_len bytes are ng = leaf_len >> 7
groups of 128 through stream_groups' two-group register ring, run to the wave's
largest count ng_wave, then rem = leaf_len & 127 bytes through finish_tail (1 to
3 blocks, the last partial word byte by byte), the constant padding block of a
full leaf, or the zero hash of an empty one.

The tree reductions (merkle_node_kernel: tiles of 512 rows, per = 512 >> K
pieces each; merkle_piece_kernel: tiles of 256, per = 256 >> K): after level L
piece q of the tile with log2w == L emits row (q << K) >> L.

  LEAF, GROUP, TILE_LOG2, PIECE_TILE_LOG2   read from the kernel sources
  GRID                 single leaf lengths
  recipes()            {name: 64 leaf lengths}: one wave each
  leaf_launches()      {entry: [lanes of one launch, ...]} for the five entries
  wave_classes, leaf_classes, check_leaf_cover
                       pure functions of lengths restating the lane's arithmetic
                       (tests/test_merkle_sweep_cpu.py asserts that no class is
                       left out)
  layout, stage_layout the bytes: pieces in one random buffer, and that buffer
                       with every byte outside the pieces inverted
  tree_shape, count_batches, wide_shape, tree_classes
                       piece counts and per-piece widths for the tree kernels
  sha256, leaf_rows, tree_root, pad_hash, layer_root
                       hashlib and the BEP 52 model

Two places where the shapes differ from the plainest reading of their recipe,
both to the stricter side:
  * a tree shape has max(2, K + 1) whole tiles, not 2: every width 0..K has
    to sit at position 0 and at position per - 1 of a whole tile, and two tiles
    have room for two widths there;
  * the lone piece of the partial tile has one width (K // 2); the count
    batches, which have no log2w, put width K there.
"""
import hashlib
import os
import random
import re

import numpy as np

from _sha1_sweep import _CSRC, _constants

_SRC = os.path.join(_CSRC, "sha256_kernels.hip")
_K = _constants(_SRC, ("kLeaf", "kTileLog2", "kPieceTileLog2"))
LEAF, TILE_LOG2, PIECE_TILE_LOG2 = _K["kLeaf"], _K["kTileLog2"], _K["kPieceTileLog2"]
GROUP = _constants(os.path.join(_CSRC, "vx_kernels.h"), ("kBlock",))["kBlock"]  # threads of a leaf workgroup
WAVE = 64
NG_FULL = LEAF >> 7  # 128 groups in a full leaf


def _ring_depth():
    with open(_SRC) as f:
        m = re.findall(r"^\s*uint4 ring\[(\d+)\]\[8\];", f.read(), re.M)
    if len(m) != 1:
        raise RuntimeError("sha256_kernels.hip: stream_groups' register ring was not found; "
                           "the sweep derives its shapes from it")
    return int(m[0])


RING = _ring_depth()
if RING != 2:
    raise RuntimeError(f"sha256_kernels.hip: stream_groups' ring is {RING} groups deep, the sweep's group counts "
                       "(parity of ng_wave, 0..6 and 125..128) were chosen for 2: rework tests/_merkle_sweep.py")

SEED = 0x52B2


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------
def sha256(b):
    return hashlib.sha256(b).digest()


ZERO = bytes(32)


def leaf_rows(data, log2_width):
    """The 2^log2_width leaf rows of a piece: a slot at or past its end is 32 zero bytes."""
    return [sha256(data[o:o + LEAF]) if o < len(data) else ZERO for o in range(0, LEAF << log2_width, LEAF)]


def tree_root(rows):
    rows = list(rows)
    while len(rows) > 1:
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
    return rows[0]


def pad_hash(height):
    h = ZERO
    for _ in range(height):
        h = sha256(h + h)
    return h


def layer_root(rows, height=0):
    """Root of a layer standing `height` levels above the leaves, each level
    padded to an even count with the pad hash of its height."""
    rows = list(rows)
    while len(rows) > 1:
        if len(rows) & 1:
            rows.append(pad_hash(height))
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
        height += 1
    return rows[0]


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ---------------------------------------------------------------------------
# leaf lengths and waves
# ---------------------------------------------------------------------------
GRID_GROUPS = (0, 1, 2, 3, NG_FULL - 2, NG_FULL - 1)
GRID = [128 * g + r for g in GRID_GROUPS for r in range(128)] + [LEAF]

# tails for the lanes of a recipe that is about group counts: every rem % 4, both sides of 55 | 56 and 119 | 120
TAILS = (0, 1, 2, 3, 4, 54, 55, 56, 57, 62, 63, 64, 65, 66, 118, 119, 120, 121, 126, 127)
UNIFORM_GROUPS = (0, 1, 2, 3, 4, 5, 6, NG_FULL - 3, NG_FULL - 2, NG_FULL - 1, NG_FULL)
LONG_GROUPS = (NG_FULL, NG_FULL - 1, 5, 4)
LONG_LANES = (0, WAVE - 1, 31)
TAIL_GROUPS = (0, 1, 2, NG_FULL - 1)
MIXED = "mixed: "  # recipes whose lanes differ in group count carry this prefix


def _len(g, r):
    return LEAF if g >= NG_FULL else 128 * g + r


def recipes():
    """{name: 64 leaf lengths}, in the order they are laid end to end."""
    out = {}
    for g in UNIFORM_GROUPS:
        out[f"uniform {g}"] = [_len(g, TAILS[(j + 3 * g) % len(TAILS)]) for j in range(WAVE)]
    for g in LONG_GROUPS:
        for lane in LONG_LANES:
            wave = [_len(j % 3, TAILS[(7 * j + g) % len(TAILS)]) for j in range(WAVE)]
            wave[lane] = _len(g, TAILS[(lane + g) % len(TAILS)])
            out[f"{MIXED}one lane of {g} groups at lane {lane}"] = wave
    up = [_len(j, TAILS[j % len(TAILS)]) for j in range(WAVE)]
    out[MIXED + "ascending"] = up
    out[MIXED + "descending"] = up[::-1]
    out["all empty"] = [0] * WAVE
    out["all tails below a group"] = [1 + (5 * j) % 127 for j in range(WAVE)]
    full = [LEAF] * WAVE
    full[40] = 0
    out[MIXED + "full leaves and one empty lane"] = full
    for g in TAIL_GROUPS:
        out[f"tails 0..63 at {g} groups"] = [128 * g + r for r in range(64)]
        out[f"tails 64..127 at {g} groups"] = [128 * g + r for r in range(64, 128)]
    assert all(len(w) == WAVE for w in out.values())
    return out


# the partial last wave: one group each (so it adds no mixed wave), the last row a two-byte partial word
LAST_WAVE = [128 + TAILS[j % len(TAILS)] for j in range(36)] + [130]


def leaf_batch(rec=None):
    """The recipes end to end and the partial last wave."""
    rec = recipes() if rec is None else rec
    lens = [L for w in rec.values() for L in w] + LAST_WAVE
    assert len(lens) % WAVE and len(lens) % GROUP
    return lens


# merkle_blocks: a lane's block has 16 KiB of the stage whatever its length, so the batch goes in launches
BLOCKS_PER_LAUNCH = 15 * WAVE  # 15 MiB of stage
BLOCKS_SKIPPED = (5, 70)  # lanes of every launch whose row is SKIP_ROW (if the launch is that long)


def blocks_launches(lens):
    """[(first lane, lengths, skipped lanes)] of the merkle_blocks launches."""
    out = []
    for at in range(0, len(lens), BLOCKS_PER_LAUNCH):
        part = lens[at:at + BLOCKS_PER_LAUNCH]
        out.append((at, part, tuple(k for k in BLOCKS_SKIPPED if k < len(part))))
    return out


# merkle_uniform: n pieces of one length and a last one of another, 0 < last_len <= len (the C entry refuses
# anything else).  Every ninth length of the grid (an even step would keep the parity of the tail), the last
# piece somewhere below it.
UNIFORM_N = 65


def uniform_pairs():
    """[(name, len, last_len, n)]: the grid walk at n = 65, where a wave holds one length, then the few waves
    this kernel can mix (n <= 64: the lanes past n redo the last piece)."""
    out = []
    for k in range(1, len(GRID), 9):
        a = GRID[k]
        # the first length from a point that moves with k whose tail class is not that of `a` (a == 1 has none)
        cands = [1 + (7 * k + 391 + d) % a for d in range(a)]
        b = next((c for c in cands if lane_classes(c) != lane_classes(a)), cands[0])
        out.append((f"grid {k}", a, b, UNIFORM_N))
    out += [(MIXED + "long first", LEAF, 130, 2), (MIXED + "long first, 127 groups", LEAF - 70, 1, 2),
            (MIXED + "half and half", 4 * 128 + 57, 128 + 3, 33), (MIXED + "full and short", LEAF, 5, 40)]
    return out


def uniform_stride(length):
    """16-byte aligned, above the length, no multiple of 128: the pieces walk the phases of a line."""
    s = (length + 15) // 16 * 16 + 16
    return s + 32 if s % 128 == 0 else s


ENTRIES = ("ragged", "uniform", "block_check", "blocks", "pieces")


def leaf_launches(fix=None, keep=None):
    """{entry: [lane lengths of one launch, ...]} at log2_width 0, as the GPU
    tests run them.  fix: applied to every length; keep: a predicate on recipe
    and pair names (both for tests/test_merkle_sweep_cpu.py's doctored shapes)."""
    fix = fix or (lambda L: L)
    keep = keep or (lambda name: True)
    rec = {name: [fix(L) for L in w] for name, w in recipes().items() if keep(name)}
    batch = [L for w in rec.values() for L in w] + [fix(L) for L in LAST_WAVE]
    blocks = []
    for _, part, skipped in blocks_launches(batch):
        blocks.append([0 if k in skipped else L for k, L in enumerate(part)])  # a skipped lane hashes nothing
    uniform = [[fix(a)] * (n - 1) + [fix(b)] for name, a, b, n in uniform_pairs() if keep(name)]
    return {"ragged": [batch], "uniform": uniform, "block_check": [batch], "blocks": blocks, "pieces": [batch]}


# ---------------------------------------------------------------------------
# classifiers
# ---------------------------------------------------------------------------
LANE_CLASSES = ("tail of 1 block", "tail of 2 blocks", "tail of 3 blocks", "rem % 4 == 0, rem > 0", "rem % 4 == 1",
                "rem % 4 == 2", "rem % 4 == 3", "rem == 0 on a short leaf", "full leaf", "empty leaf")
WAVE_CLASSES = ("ng_wave odd", "ng_wave even", "ng_wave == 0, nothing hashed", "ng_wave == 0, tails run",
                "a lane with 0 < ng < ng_wave", "a lane with ng == 0 while ng_wave > 0",
                "the one longest lane is lane 0", "the one longest lane is lane 63", "the one longest lane is inside")
# merkle_leaf_kernel<false> has one length per launch and a last piece with 0 < last_len <= len: no lane is
# empty at log2_width 0, and the one lane that differs is the last and the shorter.
UNREACHABLE = {"uniform": {"the one longest lane is inside", "the one longest lane is lane 63", "empty leaf",
                           "ng_wave == 0, nothing hashed"}}


def lane_classes(L):
    assert 0 <= L <= LEAF
    if L == 0:
        return {"empty leaf"}
    if L == LEAF:
        return {"full leaf"}
    rem = L & 127
    out = {"tail of %d block%s" % ((rem + 9 + 63) >> 6, "s" if rem > 55 else "")}
    if rem == 0:
        out.add("rem == 0 on a short leaf")
    elif rem % 4 == 0:
        out.add("rem % 4 == 0, rem > 0")
    else:
        out.add(f"rem % 4 == {rem % 4}")  # the last word is partial: finish_tail's byte loop
    return out


def wave_classes(wave):
    """The classes of one wave of 64 lanes, from the lengths alone."""
    assert len(wave) == WAVE
    ng = [L >> 7 for L in wave]
    top = max(ng)
    out = set()
    for L in wave:
        out |= lane_classes(L)
    if top == 0:
        out.add("ng_wave == 0, tails run" if any(wave) else "ng_wave == 0, nothing hashed")
        return out
    out.add("ng_wave odd" if top & 1 else "ng_wave even")
    if any(0 < g < top for g in ng):
        out.add("a lane with 0 < ng < ng_wave")
    if 0 in ng:
        out.add("a lane with ng == 0 while ng_wave > 0")
    if ng.count(top) == 1:
        at = ng.index(top)
        out.add("the one longest lane is " + ("lane 0" if at == 0 else "lane 63" if at == WAVE - 1 else "inside"))
    return out


def leaf_classes(launch):
    """The classes of a launch; the lanes past n of the last wave redo lane n - 1."""
    out = set()
    for at in range(0, len(launch), WAVE):
        w = launch[at:at + WAVE]
        out |= wave_classes(w + [launch[-1]] * (WAVE - len(w)))
    return out


def check_leaf_cover(launches):
    """Every class in the launches of every entry, or an AssertionError that names what is missing."""
    for entry in ENTRIES:
        got = set()
        for launch in launches[entry]:
            got |= leaf_classes(launch)
        want = set(LANE_CLASSES + WAVE_CLASSES) - UNREACHABLE.get(entry, set())
        left = sorted(want - got)
        assert not left, f"{entry}: classes no lane of its launches is in: {left}"
        assert got <= set(LANE_CLASSES + WAVE_CLASSES), sorted(got - set(LANE_CLASSES + WAVE_CLASSES))


# ---------------------------------------------------------------------------
# bytes
# ---------------------------------------------------------------------------
def outside_flipped(host, offs, lens):
    """A copy of host with every byte outside the pieces XORed with 0xFF."""
    delta = np.zeros(len(host) + 1, dtype=np.int64)
    np.add.at(delta, np.asarray(offs, dtype=np.int64), 1)
    np.add.at(delta, np.asarray(offs, dtype=np.int64) + np.asarray(lens, dtype=np.int64), -1)
    inside = np.cumsum(delta[:-1]) > 0
    out = host.copy()
    out[~inside] ^= 0xFF
    assert (out[inside] == host[inside]).all() and (out != host).sum() == (~inside).sum() > 0
    return out


def layout(lens, seed=SEED):
    """(offsets, host, flipped): piece i at a 16-byte aligned offset whose
    16-byte phase within a 128-byte line is i % 8, at least 16 random bytes
    between neighbours and 64 behind the last."""
    offs, o = [], 0
    for i, L in enumerate(lens):
        a = (o + 15) // 16
        a += (i % 8 - a) % 8
        offs.append(16 * a)
        o = 16 * a + L + 16
    host = random_bytes(seed + len(lens), o + 64)
    return offs, host, outside_flipped(host, offs, lens)


def overlapped_layout(lens, seed=SEED):
    """Pieces that share their bytes: piece i at offset 16 * i of one buffer as
    long as the longest needs (a batch of many pieces of a MiB each in about a
    MiB).  The bytes behind a piece's end belong to its neighbours here, so
    there is no inverted copy; a lane that read them would still miss hashlib."""
    offs = [16 * i for i in range(len(lens))]
    host = random_bytes(seed + 7 * len(lens), max(o + L for o, L in zip(offs, lens)) + 64)
    return offs, host


def stage_layout(host, offs, lens, seed=SEED):
    """(stage, flipped) for merkle_blocks: block b is the piece's bytes at
    b * 16 KiB, the rest of its 16 KiB random."""
    n = len(lens)
    stage = random_bytes(seed + 3 * n + 1, n * LEAF)
    for b, (o, L) in enumerate(zip(offs, lens)):
        stage[b * LEAF:b * LEAF + L] = host[o:o + L]
    return stage, outside_flipped(stage, [b * LEAF for b in range(n)], lens)


def hash_rows(host, offs, lens):
    """[n, 32] uint8: SHA-256 of every piece as one leaf; an empty one is the zero row."""
    view = memoryview(host)
    return np.frombuffer(b"".join(sha256(view[o:o + L]) if L else ZERO for o, L in zip(offs, lens)),
                         dtype=np.uint8).reshape(len(lens), 32).copy()


def one_bit_off(rows, every=3):
    """(expected, ok): row i one bit away, bit i % 8 of byte i % 32, for i % every == 0."""
    exp = rows.copy()
    idx = np.arange(0, len(rows), every)
    exp[idx, idx % 32] ^= (1 << (idx % 8)).astype(np.uint8)
    ok = np.ones(len(rows), dtype=np.uint8)
    ok[idx] = 0
    return exp, ok


# ---------------------------------------------------------------------------
# tree shapes
# ---------------------------------------------------------------------------
KERNELS = {"node": TILE_LOG2, "piece": PIECE_TILE_LOG2}  # rows of a tile, log2; the widths one launch covers


def per_tile(kernel, K):
    assert 0 <= K <= KERNELS[kernel]
    return (1 << KERNELS[kernel]) >> K


def tree_shape(kernel, K):
    """log2w of the n pieces of the width shape: n = t * per + 1, t the
    smallest count of whole tiles with t >= max(2, K + 1) and n >= 2 (K + 1).
    Width (k + j) % (K + 1) sits at position 0 of tile k and width (k + 1 + j)
    % (K + 1) at its position per - 1 (per > 1), so over the first K + 1 tiles
    every width is at both; the other positions cycle; the lone piece of the
    partial tile has width K // 2."""
    per = per_tile(kernel, K)
    t = max(2, K + 1)
    while t * per + 1 < 2 * (K + 1):
        t += 1
    n = t * per + 1
    lw = [(5 * i + i // per) % (K + 1) for i in range(n)]
    for k in range(t):
        lw[k * per] = k % (K + 1)
        lw[k * per + per - 1] = (k + (1 if per > 1 else 0)) % (K + 1)
    lw[n - 1] = K // 2
    return lw


def count_batches(kernel, K):
    per = per_tile(kernel, K)
    return sorted({n for n in (1, per - 1, per, per + 1) if n >= 1})


def tree_classes(kernel, K, lw):
    """What a width shape reaches: {(where, width)}."""
    per = per_tile(kernel, K)
    n = len(lw)
    out = set()
    for i, w in enumerate(lw):
        whole = (i // per + 1) * per <= n
        if not whole:
            out.add(("partial tile", w))
            continue
        if i % per == 0:
            out.add(("position 0", w))
        if i % per == per - 1:
            out.add(("position per - 1", w))
        if kernel == "node" and K == 0:  # a thread owns pieces q and q + 256 of the tile
            out.add(("first piece of a thread" if i % per < per // 2 else "second piece of a thread", w))
    return out


def check_tree_cover(kernel, K, lw):
    per = per_tile(kernel, K)
    n = len(lw)
    assert n % per == 1 % per and n // per >= 2 and n >= 2 * (K + 1), (kernel, K, n)
    assert all(0 <= w <= K for w in lw)
    got = tree_classes(kernel, K, lw)
    want = {(where, w) for where in ("position 0", "position per - 1") for w in range(K + 1)}
    if kernel == "node" and K == 0:
        want |= {("first piece of a thread", 0), ("second piece of a thread", 0)}
    left = sorted(want - got)
    assert not left, f"{kernel} kernel, log2_width {K}: not reached: {left}"
    partial = [w for where, w in got if where == "partial tile"]
    assert partial == ([lw[-1]] if per > 1 else []), "the partial tile holds one lone piece"


def piece_len(i, w, full=False):
    """Bytes of piece i of width w in a piece-kernel batch: the whole tree,
    but every eleventh piece empty and every fifth one byte more than half."""
    if full:
        return LEAF << w
    if i % 11 == 10:
        return 0
    if i % 5 == 4:
        return (LEAF << w) // 2 + 1
    return LEAF << w


WIDE = (PIECE_TILE_LOG2 + 1, PIECE_TILE_LOG2 + 2)  # widths merkle_pieces takes in two launches


def wide_shape(K):
    """[(log2w, bytes)] for K in WIDE: one piece of every width in a shuffled
    order, the widest not first (and always whole), then one more of width K
    with one byte in its second 256-leaf tile."""
    ws = list(range(K + 1))
    random.Random(SEED + K).shuffle(ws)
    if ws[0] == K:
        ws[0], ws[1] = ws[1], ws[0]
    out = [(w, piece_len(i, w, full=(w == K))) for i, w in enumerate(ws)]
    return out + [(K, (LEAF << PIECE_TILE_LOG2) + 1)]


class Pieces:
    """A batch of pieces for the leaf + tree entries and what BEP 52 says
    about it: leaves [n << K, 32] and roots [n, 32] (piece i's root is the
    root of its first 2^log2w[i] rows)."""

    def __init__(self, K, lw, lens, seed=SEED, overlapped=False):
        self.K, self.lw, self.lens, self.n = K, list(lw), list(lens), len(lens)
        assert all(L <= LEAF << w for L, w in zip(self.lens, self.lw))
        if overlapped:
            self.offs, self.host = overlapped_layout(self.lens, seed + K)
            self.flipped = None
        else:
            self.offs, self.host, self.flipped = layout(self.lens, seed + K)
        view = memoryview(self.host)
        W = 1 << K
        leaves, roots = [], []
        for o, L, w in zip(self.offs, self.lens, self.lw):
            rows = leaf_rows(view[o:o + L], K)
            leaves += rows
            roots.append(tree_root(rows[:1 << w]))
        assert len(leaves) == self.n * W
        self.leaves = np.frombuffer(b"".join(leaves), dtype=np.uint8).reshape(self.n * W, 32).copy()
        self.roots = np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(self.n, 32).copy()


def piece_batch(K):
    """The width shape of the piece kernel at K <= 8, or the wide shape above."""
    if K in WIDE:
        shape = wide_shape(K)
        return Pieces(K, [w for w, _ in shape], [L for _, L in shape])
    lw = tree_shape("piece", K)
    return Pieces(K, lw, [piece_len(i, w) for i, w in enumerate(lw)])


def node_rows(K, lw, seed=SEED):
    """(rows, flipped, roots): random rows for all n << K rows; in the copy
    the rows behind a piece's first 2^log2w are inverted."""
    n, W = len(lw), 1 << K
    rows = random_bytes(seed + 100 + K + n, n * W * 32).reshape(n * W, 32)
    flipped = rows.copy()
    roots = []
    for i, w in enumerate(lw):
        flipped[i * W + (1 << w):(i + 1) * W] ^= 0xFF
        roots.append(tree_root([rows[i * W + k].tobytes() for k in range(1 << w)]))
    return rows, flipped, np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(n, 32).copy()
