"""Shapes for the two kernels that hash zeros from nothing, sha1_zero_kernel
(sha1_tail_kernels.hip) and merkle_zero_leaf_kernel (sha256_kernels.hip), and a
model of which path of a kernel a lane takes.  Host only: no torch, no library.

Both kernels run z = len >> 6 all-zero blocks to the wave's largest count under
a select, then build the last one or two blocks from rem = len & 63 (the 0x80
at byte rem & 3 of word rem >> 2, the bit length).  The leaf kernel besides
scatters through a row table and, given the full block's row, stores it as is
for lanes of 16384 bytes ("known" lanes, which then count as z = 0) and skips
the last compression in a wave of known lanes only.

  SHA1_*          length lists for sha1_zero_kernel: one launch each
  LEAF_*          length lists for merkle_zero_leaf_kernel
  leaf_lens(n)    the n lanes of the table / full-row product
  rows_table      the three forms of the row table
  class_sha1, class_leaf
                  pure functions restating a kernel's arithmetic for one lane
                  of one wave (tests/test_zero_sweep_cpu.py asserts that the
                  shapes reach every class that can be reached)
  sha1_of_zeros, sha256_of_zeros
                  hashlib, once per distinct length
"""
import functools
import hashlib
import os
import random

from _sha1_sweep import _CSRC, _constants

WAVE = 64
SHA1_GROUP = _constants(os.path.join(_CSRC, "sha1_tail_kernels.hip"), ("kTailBlock",))["kTailBlock"]
LEAF_GROUP = _constants(os.path.join(_CSRC, "vx_kernels.h"), ("kBlock",))["kBlock"]
LEAF = _constants(os.path.join(_CSRC, "sha256_kernels.hip"), ("kLeaf",))["kLeaf"]

SEED = 0x2E70


def shuffled(lens, seed=SEED):
    out = list(lens)
    random.Random(seed).shuffle(out)
    return out


def waves_of(lens, width=WAVE):
    return [lens[k:k + width] for k in range(0, len(lens), width)]


@functools.lru_cache(maxsize=None)
def sha1_of_zeros(n):
    return hashlib.sha1(bytes(n)).digest()


@functools.lru_cache(maxsize=None)
def sha256_of_zeros(n):
    return hashlib.sha256(bytes(n)).digest()


# ---------------------------------------------------------------------------
# sha1_zero_kernel
# ---------------------------------------------------------------------------
# every rem at z = 0..4 (so every rem & 3, both sides of 55 | 56, the empty message); in order: 321
# lanes are five waves of one z each and one lane, so lanes past n run
SHA1_GRID = list(range(321))
SHA1_SHUFFLED = shuffled(SHA1_GRID)  # every wave mixes block counts
SHA1_SHORT = (0, 1, 58, 62)  # rem & 3 of 0, 1, 2, 2 on both sides of no block at all
SHA1_LONG_LENS = (4095, 4096, 65535, 65536, 65537, 262144, (1 << 20) + 57)


def _sha1_long():
    """A wave per long length, the short lanes filling it (their finished state
    sits under the select for all of the long lane's blocks), then a wave
    with all of them."""
    out = []
    for k, L in enumerate(SHA1_LONG_LENS):
        wave = [SHA1_SHORT[(j + k) % len(SHA1_SHORT)] for j in range(WAVE)]
        wave[(11 * k + 5) % WAVE] = L
        out += wave
    return out + list(SHA1_SHORT) + list(SHA1_LONG_LENS)


SHA1_LONG = _sha1_long()
SHA1_HUGE_LEN = 4 << 20  # 65,536 blocks in one lane
SHA1_HUGE = [0, 1, SHA1_HUGE_LEN, 58, 62, 119, 4096]


def class_sha1(length, wave, full=False):
    """(min(z, 2), rem, two padding blocks, below the wave's largest z, known,
    the wave's kind); no lane of this kernel is known."""
    z = length >> 6
    return (min(z, 2), length & 63, (length & 63) > 55, z < max(L >> 6 for L in wave), False, "none")


# ---------------------------------------------------------------------------
# merkle_zero_leaf_kernel
# ---------------------------------------------------------------------------
LEAF_TOP = list(range(LEAF - 65, LEAF + 1))  # the last remainders at 255 blocks, and the full block
LEAF_GRID = list(range(1, 192)) + LEAF_TOP  # every rem at z = 0, 1 and 2
LEAF_SHUFFLED = shuffled(LEAF_GRID)
LEAF_NS = (1, 63, 64, 65, 257, 300)  # the workgroup is LEAF_GROUP = 256 threads


def _leaf_master():
    """The lanes of the table / full-row product, leaf_lens(n) its first n:
    wave 0   1..63 (no zero block at all: n = 1 and n = 63), then one full lane
    wave 1   full lanes only (n = 65: one live lane)
    wave 2   63 full lanes and one of 16383 bytes
    wave 3   no full lane
    lane 256 the second workgroup's first, a full lane; the rest mixed."""
    rng = random.Random(SEED + 1)
    m = list(range(1, 64)) + [LEAF]
    m += [LEAF] * WAVE
    m += [LEAF] * WAVE
    m[2 * WAVE + 22] = LEAF - 1
    m += shuffled([L for L in LEAF_GRID if L != LEAF], SEED + 2)[:WAVE]
    m += [LEAF] + [LEAF if rng.random() < 0.4 else rng.choice(LEAF_GRID) for _ in range(LEAF_NS[-1] - 4 * WAVE - 1)]
    assert len(m) == LEAF_NS[-1]
    return m


LEAF_MASTER = _leaf_master()


def leaf_lens(n):
    return LEAF_MASTER[:n]


def _leaf_cover():
    """Waves for what the other lists leave out: every rem of one band of z
    (0, 1, 2) beside full lanes and nothing longer, so with a full row given
    those lanes are the wave's longest, and without it the full lanes are."""
    out = []
    for z in (0, 1, 2):
        for odd in (0, 1):
            band = [64 * z + r for r in range(odd, 64, 2) if 64 * z + r]
            wave = [LEAF] * WAVE
            wave[odd:2 * len(band):2] = band
            out += wave
    out += list(range(64, 128))  # no full lane and one block each: no lane is below the wave's count
    # every length beside full lanes and longer ones: below the wave's count in a mixed wave
    for k, L in enumerate(shuffled(LEAF_GRID[:-1], SEED + 3)):
        out += [L, LEAF] if k % 3 == 2 else [L]
    return out + [LEAF - 2]  # (a last wave of one live lane)


LEAF_COVER = _leaf_cover()

ROWS_FORMS = ("none", "permuted", "gaps")
FULL_FORMS = ("none", "true", "c3")


def rows_table(form, n, seed=SEED):
    """(rows or None, rows of the output): `none` is row j; `permuted` a seeded
    permutation of 0..n-1; `gaps` strictly increasing with gaps, so the output
    has more rows than lanes."""
    if form == "none":
        return None, n
    rng = random.Random(seed + n)
    if form == "permuted":
        rows = list(range(n))
        rng.shuffle(rows)
        return rows, n
    assert form == "gaps"
    rows, r = [], rng.randrange(3)
    for _ in range(n):
        rows.append(r)
        r += rng.choice((1, 1, 2, 5))
    return rows, r + 3


def full_row(form):
    """The full_row argument: None, the true SHA-256 of 16,384 zeros, or 32
    bytes of 0xC3 (not a hash: tells "stored as is" from "hashed anyway")."""
    return {"none": None, "true": sha256_of_zeros(LEAF), "c3": b"\xc3" * 32}[form]


def leaf_want(lens, full):
    """The leaf rows of a launch, lane by lane."""
    return [full if full is not None and L == LEAF else sha256_of_zeros(L) for L in lens]


def class_leaf(length, wave, full):
    """The class of a lane of merkle_zero_leaf_kernel, as class_sha1: a known
    lane (full row given, 16384 bytes) counts as z = 0."""
    def z_of(L):
        return 0 if full and L == LEAF else L >> 6

    known = [bool(full) and L == LEAF for L in wave]
    kind = "all" if all(known) else "mixed" if any(known) else "none"
    z = z_of(length)
    return (min(z, 2), length & 63, (length & 63) > 55, z < max(z_of(L) for L in wave), bool(full) and length == LEAF,
            kind)


def leaf_launches():
    """(what, lengths, full row given) of every launch of the leaf kernel in
    tests/test_gpu_zero_sweep.py."""
    out = [("grid", LEAF_GRID, False), ("shuffled", LEAF_SHUFFLED, False)]
    for full in (False, True):
        out.append((f"cover, full {full}", LEAF_COVER, full))
        out += [(f"n {n}, full {full}", leaf_lens(n), full) for n in LEAF_NS]
    return out


def sha1_launches():
    return [("grid", SHA1_GRID), ("shuffled", SHA1_SHUFFLED), ("long", SHA1_LONG), ("huge", SHA1_HUGE)]


def classes(fn, lens, full=False):
    """The classes of every lane of a launch; the lanes past n of the last wave
    redo lane n - 1."""
    out = set()
    for w in waves_of(list(lens)):
        w = w + [lens[-1]] * (WAVE - len(w))
        out |= {fn(L, w, full) for L in w}
    return out


def missing(reachable, got, what):
    left = sorted(reachable - got)
    assert not left, f"{what}: {len(left)} of {len(reachable)} reachable classes are not covered: {left}"
    assert got <= reachable, f"{what}: classes outside the brute-force set: {sorted(got - reachable)}"
