"""Shapes for gather_kernel (vortex_amd/csrc/vx_gather.hip) on its own, a model
of its result and a classifier of which path a tile and a launch take.  Host
only: no torch, no library; numpy for the bytes.

The kernel: workgroup b takes tiles b, b + grid, b + 2 grid, ... of the launch
(grid = min(ntiles, cap), cap = max_grid or kGatherGrid); it finds a tile's
piece by binary search on the prefix tfirst (the last piece p with tfirst[p] <=
t: pieces that own no tile share their successor's entry and are never chosen),
copies the tile's len / 16 words with kGatherBlock threads, U words in flight
per thread, so one trip of the loop moves kGatherBlock * U words, and its
len % 16 tail bytes one per thread.

  TILE, BLOCK, GRID, U   read from vx_gather.hip
  SHAPES                 {name: [(length, gathered), ...]}: one launch each
  MAX_GRIDS              the max_grid values every shape runs with
  layout(shape, name)    sources, destinations, tfirst, source bytes
  model(lay)             the arena after the launch: numpy slice copies into 0xA5
  tile_class, piece_classes, launch_class
                         pure functions restating the kernel's index arithmetic
                         (tests/test_gather_sweep_cpu.py asserts that the shapes
                         leave no class out)
  locate(lay, at)        which piece, tile and class an arena byte belongs to
"""
import os
import re
import zlib

import numpy as np

from _sha1_sweep import _CSRC

FILL = 0xA5
SLACK = 4096  # untouched bytes before the first and behind the last destination


def _constants(path, names):
    """As _sha1_sweep._constants, for constants written as a product (64 * 1024)."""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in names:
        m = re.findall(r"^\s*constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\d+(?:\s*\*\s*\d+)*)\s*;" % name, text, re.M)
        if len(m) != 1:
            raise RuntimeError(f"{os.path.basename(path)}: expected one definition of {name}, found {len(m)}; "
                               "the sweep derives its shapes from it")
        out[name] = int(np.prod([int(x) for x in m[0].split("*")]))
    return out


_K = _constants(os.path.join(_CSRC, "vx_gather.hip"), ("kGatherTile", "kGatherBlock", "kGatherGrid", "U"))
TILE, BLOCK, GRID, U = _K["kGatherTile"], _K["kGatherBlock"], _K["kGatherGrid"], _K["U"]
TRIP = BLOCK * U  # words one trip of the unrolled loop moves
FULL = TILE // 16  # words of a full tile
MAX_GRIDS = (0, 1, 128)  # the engine passes 0 and 128; 1 makes the stride loop as long as it gets

WORD_CLASSES = ("0", "<block", "=block", "block..trip", "=trip", "trips+partial", "whole trips", "full tile")
TAIL_CLASSES = ("0", "1", "2..14", "15")
PIECE_CLASSES = ("0: empty", "0: not gathered", "1", "2", "5", "multiple of the tile")
TILELESS_AT = ("first", "middle run", "last")
N_CLASSES = ("1", "2", "3", "2^k", "2^k-1", "2^k+1")
GRID_CLASSES = ("below", "equal", "one above", "twice and one")


def cap_of(max_grid):
    return max_grid if max_grid else GRID


def tiles_of(length):
    return (length + TILE - 1) // TILE


# ---------------------------------------------------------------------------
# classifiers
# ---------------------------------------------------------------------------
def tile_class(length, k):
    """(words class, tail class) of tile k of a piece of `length` bytes."""
    ln = min(TILE, length - k * TILE)
    assert 0 < ln <= TILE
    words, tail = ln // 16, ln % 16
    if words == 0:
        w = "0"
    elif words < BLOCK:
        w = "<block"
    elif words == BLOCK:
        w = "=block"
    elif words < TRIP:
        w = "block..trip"
    elif words == TRIP:
        w = "=trip"
    elif words == FULL:
        w = "full tile"
    elif words % TRIP:
        w = "trips+partial"
    else:
        w = "whole trips"
    t = "0" if tail == 0 else "1" if tail == 1 else "15" if tail == 15 else "2..14"
    return w, t


def piece_classes(length, gathered):
    out = set()
    if length == 0:
        out.add("0: empty")
    elif not gathered:
        out.add("0: not gathered")
    else:
        k = tiles_of(length)
        if k in (1, 2, 5):
            out.add(str(k))
        if length % TILE == 0:
            out.add("multiple of the tile")
    return out


def owns_tiles(length, gathered):
    return bool(gathered and length)


def launch_class(shape, max_grid):
    """What one launch reaches beyond its tiles: {"n", "grid", "tileless"}."""
    n = len(shape)
    out = {"n": set(), "grid": set(), "tileless": set()}
    if n in (1, 2, 3):
        out["n"].add(str(n))
    if n >= 4 and n & (n - 1) == 0:
        out["n"].add("2^k")
    if n >= 4 and (n + 1) & n == 0:
        out["n"].add("2^k-1")
    if n >= 5 and (n - 1) & (n - 2) == 0:
        out["n"].add("2^k+1")
    ntiles, cap = sum(tiles_of(L) for L, g in shape if g), cap_of(max_grid)
    for name, at in (("below", cap - 1), ("equal", cap), ("one above", cap + 1), ("twice and one", 2 * cap + 1)):
        if ntiles == at:
            out["grid"].add(name)
    if ntiles:  # (a launch of no tile runs no search)
        own = [owns_tiles(L, g) for L, g in shape]
        if not own[0]:
            out["tileless"].add("first")
        if not own[-1]:
            out["tileless"].add("last")
        first, last = own.index(True), n - 1 - own[::-1].index(True)
        run = 0
        for k in range(first, last + 1):
            run = 0 if own[k] else run + 1
            if run >= 2:
                out["tileless"].add("middle run")
    return out


def search(tfirst, n, t):
    """The kernel's binary search, step for step."""
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tfirst[mid] <= t:
            lo = mid
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _last_tile_lengths():
    """A last tile's length for every (words class, tail class) there is."""
    out = []
    for words in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + BLOCK, 2 * TRIP,
                  FULL - TRIP, FULL - 1):
        for tail in (0, 1, 7, 15):
            if words or tail:
                out.append(16 * words + tail)
    return out + [TILE]


def _cover():
    """About 70 pieces that reach every class of tile and of piece: every last
    tile of _last_tile_lengths as a one-tile piece or behind one, two or four
    full tiles, empty and skipped pieces first, last and in runs; 129 tiles,
    which is twice the default grid and one."""
    shape = [(0, True), (4096 + 3, False)]  # tileless first: an empty piece, then one the launch does not gather
    lasts = _last_tile_lengths()
    fulls = {3: 1, 9: 4, 17: 1, 24: 2, 30: 4, 38: 1, 45: 2}  # full tiles in front of some of the last tiles
    for k, L in enumerate(lasts):
        shape.append((fulls.get(k, 0) * TILE + L, True))
        if k % 13 == 5:
            shape += [(0, True), (100 + k, False)]  # a run of two in the middle
        if k == 20:
            shape += [(777, False), (0, True), (TILE + 16, False)]  # a run of three
    shape += [(2 * TILE, True), (5 * TILE, True)]  # exact multiples of the tile
    spare = 2 * GRID + 1 - sum(tiles_of(L) for L, g in shape if g)
    assert spare >= 5, spare
    # the rest as five-tile pieces with a short last tile, then one-tile pieces
    k = 0
    while spare >= 5 and k < 9:
        shape.append((4 * TILE + 16 * (k + 1) + k, True))
        spare -= 5
        k += 1
    shape += [(48 + 5 * j, True) for j in range(spare)]
    return shape + [(333, False), (0, True)]  # tileless last


def _tiles_shape(ntiles):
    """A table of exactly ntiles tiles, most of them short one-tile pieces (so
    the bytes stay few), with two- and five-tile pieces, exact multiples and
    tileless pieces spread through it."""
    shape, left, k = [], ntiles, 0
    while left:
        if k % 16 == 3 and left >= 5:
            L = 4 * TILE + 16 * 37 + 9
        elif k % 16 == 8 and left >= 2:
            L = TILE + 1
        elif k % 16 == 12 and left >= 2:
            L = 2 * TILE
        else:
            L = 16 * (1 + k % 40) + (k * 7) % 16
        shape.append((L, True))
        left -= tiles_of(L)
        if k % 9 == 4:
            shape.append((0, True) if k % 2 else (5000 + k, False))
        k += 1
    return shape or [(0, True), (4000, False), (0, True)]  # ntiles 0: nothing but tileless pieces


def _n_shapes():
    """Tables of 1, 2, 3, 7, 8 and 9 pieces; with n = 1 the search loop never
    runs.  Tileless pieces stand first, last and as a run in the middle."""
    return {
        "n1": [(3 * TILE + 5, True)],
        "n1 one word": [(16, True)],
        "n2": [(TILE + 1, True), (15, True)],
        "n2 tileless first": [(0, True), (2 * TILE, True)],
        "n3": [(31, True), (900, False), (5 * TILE - 1, True)],
        "n3 tileless last": [(TILE, True), (17, True), (0, True)],
        "n7": [(1, True), (0, True), (0, True), (TILE + 15, True), (16 * BLOCK, True), (TILE - 1, True), (40, False)],
        "n8": [(4000, False), (16 * TRIP, True), (2 * TILE + 7, True), (0, True), (9000, False), (0, True), (33, True),
               (16 * TRIP + 16 * BLOCK + 1, True)],
        "n9": [(TILE, True), (0, True), (50, False), (2, True), (5 * TILE, True), (16 * (TRIP + 1), True), (47, True),
               (0, True), (TILE + 16, True)],
        # whole tiles only: a search that chose a tile's predecessor would find no byte left in it and
        # copy nothing, so this table shows such a search without an access outside a piece
        "n8 whole tiles": [(TILE, True), (0, True), (2 * TILE, True), (TILE, True), (0, True), (0, True),
                           (3 * TILE, True), (TILE, True)],
    }


def _shapes():
    out = {"cover": _cover()}
    out.update(_n_shapes())
    for k in sorted({c + d for c in map(cap_of, MAX_GRIDS) for d in (-1, 0, 1)} | {2 * cap_of(g) + 1 for g in MAX_GRIDS}):
        out[f"tiles {k}"] = _tiles_shape(k)
    return out


SHAPES = _shapes()
DESCENDING = ("cover", "n9")  # destinations in descending order of the table


# ---------------------------------------------------------------------------
# layout and model
# ---------------------------------------------------------------------------
class Layout:
    """One launch's tables and bytes.  src holds offsets into the source bytes
    (-1: the piece is not gathered, its address is 0); dst offsets into the
    arena."""

    def __init__(self, name, shape):
        rng = _rng(name)
        n = len(shape)
        self.name, self.shape, self.n = name, shape, n
        self.lens = [L for L, _ in shape]
        self.gathered = [g for _, g in shape]
        # tfirst: ceil(len / tile), accumulated over the gathered pieces only
        self.tfirst = [0]
        for L, g in shape:
            self.tfirst.append(self.tfirst[-1] + (tiles_of(L) if g else 0))
        self.ntiles = self.tfirst[-1]
        # destinations: 16-byte aligned, 16 to 272 bytes apart, in an order of their own; every piece has
        # one, the pieces that are not gathered too (it must stay as it was)
        order = list(range(n))[::-1] if name in DESCENDING else rng.permutation(n).tolist()
        self.dst, at = [0] * n, SLACK
        for i in order:
            self.dst[i] = at
            at += (self.lens[i] + 15) // 16 * 16 + 16 * int(rng.integers(1, 18))
        self.arena_bytes = at + SLACK
        # sources: 16-byte aligned, in an order unrelated to the destinations; the last one ends on the
        # source's last byte
        live = [i for i in range(n) if self.gathered[i]]
        sorder = [live[j] for j in rng.permutation(len(live)).tolist()]
        nz = [i for i in sorder if self.lens[i]]
        if nz:  # a piece with bytes goes last, one with a tail if there is one
            tailed = [i for i in nz if self.lens[i] % 16] or nz
            sorder.remove(tailed[-1])
            sorder.append(tailed[-1])
        self.src, at = [-1] * n, 0
        for j, i in enumerate(sorder):
            at = (at + 15) // 16 * 16 + (16 * int(rng.integers(0, 4)) if j else 0)
            self.src[i] = at
            at += self.lens[i]
        self.src_bytes = max(at, 16)
        # two pieces read the same source bytes: the shortest multi-word piece reads the start of the longest
        self.shared = None
        cand = sorted((i for i in live if self.lens[i] >= 16 and i != (sorder[-1] if sorder else -1)),
                      key=lambda i: self.lens[i])
        if len(cand) >= 2:
            self.src[cand[0]] = self.src[cand[-1]]
            self.shared = (cand[0], cand[-1])
        # no source byte is the arena's fill byte, so a byte that was not copied always shows
        data = rng.integers(0, 255, self.src_bytes, dtype=np.uint8)
        data[data >= FILL] += 1
        self.data = data

    def tables(self, src_base):
        """(src, dst_off, lens, tfirst) as numpy arrays, the sources at src_base."""
        src = np.array([src_base + s if s >= 0 else 0 for s in self.src], dtype=np.uint64)
        return (src, np.array(self.dst, dtype=np.uint64), np.array(self.lens, dtype=np.uint32),
                np.array(self.tfirst, dtype=np.uint32))


_layouts = {}


def layout(name):
    if name not in _layouts:
        _layouts[name] = Layout(name, SHAPES[name])
    return _layouts[name]


def model(lay):
    """The arena after the launch: slice copies into an arena of 0xA5."""
    arena = np.full(lay.arena_bytes, FILL, dtype=np.uint8)
    for i in range(lay.n):
        if lay.gathered[i] and lay.lens[i]:
            arena[lay.dst[i]:lay.dst[i] + lay.lens[i]] = lay.data[lay.src[i]:lay.src[i] + lay.lens[i]]
    return arena


def locate(lay, at):
    """Where arena byte `at` lies, in words: its piece, tile, offset within the
    tile and the tile's class, or the gap it lies in."""
    for i in range(lay.n):
        if lay.dst[i] <= at < lay.dst[i] + lay.lens[i]:
            if not lay.gathered[i]:
                return (f"piece {i} (len {lay.lens[i]}), which is not gathered: byte {at - lay.dst[i]} of its "
                        "would-be destination")
            k, off = divmod(at - lay.dst[i], TILE)
            w, t = tile_class(lay.lens[i], k)
            return (f"piece {i} (len {lay.lens[i]}, {tiles_of(lay.lens[i])} tiles), tile {k} of the piece (tile "
                    f"{lay.tfirst[i] + k} of {lay.ntiles}), offset {off} within the tile, class: words {w}, tail {t}")
    before = [i for i in range(lay.n) if lay.dst[i] + lay.lens[i] <= at]
    if not before:
        return f"the slack in front of every destination (byte {at})"
    i = max(before, key=lambda i: lay.dst[i] + lay.lens[i])
    past = at - lay.dst[i] - lay.lens[i]
    k = max(tiles_of(lay.lens[i]) - 1, 0)
    cls = "words {}, tail {}".format(*tile_class(lay.lens[i], k)) if lay.lens[i] else "no tile"
    return (f"no destination: {past} bytes past the end of piece {i} (len {lay.lens[i]}, gathered "
            f"{lay.gathered[i]}), whose last tile is tile {k} of the piece, offset {lay.lens[i] - k * TILE + past} "
            f"within it, class: {cls}")


def first_difference(lay, got, want):
    """None, or the message for the first arena byte that differs."""
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return None
    at = int(bad[0])
    return (f"{lay.name}: {bad.size} arena bytes differ from the model, first at {at} (got {int(got[at]):#04x}, want "
            f"{int(want[at]):#04x}): {locate(lay, at)}")


# ---------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------
def covered(shapes=None, max_grids=MAX_GRIDS):
    """Every class the launches of tests/test_gpu_gather_sweep.py reach."""
    shapes = SHAPES if shapes is None else shapes
    out = {"words": set(), "tail": set(), "tile": set(), "piece": set(), "n": set(), "tileless": set(),
           "grid": {g: set() for g in max_grids}}
    for shape in shapes.values():
        for L, g in shape:
            out["piece"] |= piece_classes(L, g)
            if owns_tiles(L, g):
                for k in range(tiles_of(L)):
                    w, t = tile_class(L, k)
                    out["words"].add(w)
                    out["tail"].add(t)
                    out["tile"].add((w, t))
        for g in max_grids:
            c = launch_class(shape, g)
            out["n"] |= c["n"]
            out["tileless"] |= c["tileless"]
            out["grid"][g] |= c["grid"]
    return out


def missing(got):
    """The classes of the module's lists that `got` leaves out, as strings."""
    left = [f"words {w}" for w in WORD_CLASSES if w not in got["words"]]
    left += [f"tail {t}" for t in TAIL_CLASSES if t not in got["tail"]]
    left += [f"tile ({w}, {t})" for w in WORD_CLASSES[:-1] for t in TAIL_CLASSES
             if (w, t) != ("0", "0") and (w, t) not in got["tile"]]
    left += [f"piece {p}" for p in PIECE_CLASSES if p not in got["piece"]]
    left += [f"n {c}" for c in N_CLASSES if c not in got["n"]]
    left += [f"tileless {c}" for c in TILELESS_AT if c not in got["tileless"]]
    left += [f"max_grid {g}: ntiles {c} the cap" for g, s in got["grid"].items() for c in GRID_CLASSES if c not in s]
    return left
