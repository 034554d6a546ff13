"""Batches of hash proofs for merkle_proof_span_kernel / merkle_proof_walk_kernel
(vortex_amd/csrc/sha256_kernels.hip) and their hashlib results.  Host only: no
torch, no library.  The model is `walk` of tests/test_merkle_layers_cpu.py (a
receiver's check of one `hashes` message, ten lines of hashlib); the builders
here only choose descriptors and lay rows out.

The walk kernel runs kBlock = 256 lanes a workgroup, one proof a lane; its loop
bound is the wave's largest uncle count, and lanes past the last proof redo it
and store nothing.  So the batches are chosen by lane: sizes either side of a
wave and of a workgroup, named distributions of the uncle counts over the lanes
of a wave, rows that several proofs share, expected rows one bit off, and bad
descriptors among good neighbours.

  Batch           rows, proofs (pos, row, expected, span, uncles), expected rows, tops
  size_batch(n)   n proofs: spans cycle 1..512, uncles from UNCLE_MIX, 64-bit pos
  wave_batch(k)   130 proofs whose uncle counts follow WAVE_SHAPES[k]
  shared_batch()  proofs that name the same rows and one expected row
  one_bit_batch() 256 proofs, expected row i one bit off at bit i
  bad_batch(fill) 300 proofs with bad descriptors at BAD_AT
  far_proofs()    the four proofs behind the 4 GiB line and their rows
"""
import functools
import random

from test_merkle_layers_cpu import model_root, walk

WAVE = 64
SIZES = (1, 63, 64, 65, 255, 256, 257, 600)
SPANS = tuple(1 << k for k in range(10))  # 1 .. 512
UNCLE_MIX = (64, 0, 1, 63, 5, 32, 64, 17, 2, 40, 9)  # 11 entries against 10 spans: every pairing comes up
WAVE_N = 130  # two waves and a partial one of two lanes


class Batch:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.rows, self.proofs, self.expected, self.tops = [], [], [], []

    def add(self, span, uncles, pos, row=None, expected=None):
        """A proof over rows of its own (row None: appended) or over rows
        already there; its expected row is its true top (expected None: a row
        of its own) or the row given by index."""
        if row is None:
            row = len(self.rows)
            self.rows += [self.rng.randbytes(32) for _ in range(span + uncles)]
        assert row + span + uncles <= len(self.rows)
        top = walk(b"".join(self.rows[row:row + span + uncles]), span, uncles, pos)
        if expected is None:
            expected = len(self.expected)
            self.expected.append(top)
        self.proofs.append((pos, row, expected, span, uncles))
        self.tops.append(top)
        return top

    @property
    def n(self):
        return len(self.proofs)

    def verdicts(self):
        return [1 if self.expected[p[2]] == t else 0 for p, t in zip(self.proofs, self.tops)]


def _pos(rng, force_top_bit=False):
    pos = rng.getrandbits(64)
    return pos | 1 << 63 if force_top_bit else pos


@functools.lru_cache(maxsize=None)
def size_batch(n):
    b = Batch(0x5127 + n)
    forced = False
    for i in range(n):
        uncles = UNCLE_MIX[i % len(UNCLE_MIX)]
        b.add(SPANS[i % len(SPANS)], uncles, _pos(b.rng, uncles == 64 and not forced))
        forced |= uncles == 64
    assert forced and any(p[4] == 64 and p[0] >> 63 for p in b.proofs)
    return b


def _one_at(*lanes):
    return lambda i: 64 if i in lanes else 0


WAVE_SHAPES = {
    "no uncles": lambda i: 0,                       # the loop never runs
    "all 64": lambda i: 64,
    "64 at lane 0": _one_at(0, WAVE, 2 * WAVE),     # lane 0 of every wave
    "64 at lane 63": _one_at(WAVE - 1, 2 * WAVE - 1),
    "64 at the last live lane": _one_at(WAVE_N - 1),
    "descending": lambda i: WAVE - i % WAVE,        # 64 .. 1 within a wave
    "ascending": lambda i: 1 + i % WAVE,            # 1 .. 64: the longest lane is the last live one
}


@functools.lru_cache(maxsize=None)
def wave_batch(name):
    b = Batch(0x3A7E + sorted(WAVE_SHAPES).index(name))
    count = WAVE_SHAPES[name]
    for i in range(WAVE_N):
        b.add(SPANS[(3 * i) % len(SPANS)] if i % 4 else 1, count(i), _pos(b.rng, count(i) == 64))
    return b


@functools.lru_cache(maxsize=None)
def shared_batch():
    """Over one block of 700 rows: proofs with the same `row` (the same
    descriptor, another pos, another span or uncle count), ranges that overlap,
    40 proofs that name expected row 0 (24 of them reach it), and proofs with
    expected rows of their own."""
    b = Batch(0x54A2ED)
    b.rows = [b.rng.randbytes(32) for _ in range(700)]
    pos0 = b.rng.getrandbits(64)
    b.add(4, 9, pos0, row=0)  # expected row 0
    for k in range(24):
        b.add(4, 9, pos0, row=0, expected=0)  # the same descriptor: the same top
    for k in range(15):
        b.add(4, 9, pos0 ^ 1 << (k % 9), row=0, expected=0)  # another side somewhere: not row 0
    for span, uncles in ((8, 9), (4, 10), (1, 0), (2, 64), (512, 64)):
        b.add(span, uncles, b.rng.getrandbits(64), row=0)  # the same row, other shapes
    for k in range(60):  # overlapping ranges, a few rows apart
        span = SPANS[k % 8]
        b.add(span, (7 * k) % 65, b.rng.getrandbits(64), row=3 * k + k % 2)
    assert b.n == 105 and b.verdicts().count(0) == 15 and sum(1 for p in b.proofs if p[2] == 0) == 40
    return b


@functools.lru_cache(maxsize=None)
def one_bit_batch():
    """256 proofs; wrong_expected()[i] is proof i's top with bit i of its 256 flipped."""
    b = Batch(0xB17)
    for i in range(256):
        uncles = UNCLE_MIX[(i + 4) % len(UNCLE_MIX)]
        b.add(SPANS[i % 5], uncles, b.rng.getrandbits(64))
    assert [p[2] for p in b.proofs] == list(range(256))
    return b


def wrong_expected(b):
    out = []
    for i, row in enumerate(b.expected):
        row = bytearray(row)
        row[i // 8] ^= 1 << (i % 8)
        out.append(bytes(row))
    return out


# (span, uncles) of the descriptors both kernels must refuse, by proof index: lane 0, the last lane of a
# wave, the first of the next, inside a wave, either side of the workgroup edge, and the batch's last
BAD_AT = {0: (0, 3), 63: (3, 2), 64: (768, 0), 130: (1024, 1), 191: (4, 65), 255: (2, 255), 256: (0, 255),
          299: (3, 65)}
BAD_N = 300
BAD_GUARD = 1024 + 255  # the rows the longest bad descriptor names


@functools.lru_cache(maxsize=None)
def bad_batch(fill, zero_expected):
    """300 proofs, those at BAD_AT bad; the rows a bad descriptor names are a
    guard block of `fill` bytes in the middle of the tensor (in bounds).  A
    bad proof's expected row is row 0 of the table, or with zero_expected the
    zero row, which a zero top must not match either.  The good proofs and
    their rows do not depend on `fill`."""
    b = Batch(0xBAD)
    good_rows = []
    for i in range(BAD_N):
        if i not in BAD_AT:
            uncles = UNCLE_MIX[(i + 1) % len(UNCLE_MIX)]
            b.add(SPANS[i % 7], uncles, b.rng.getrandbits(64))
            good_rows.append(len(b.proofs) - 1)
    half = b.proofs[len(b.proofs) // 2][1]  # (where a proof's rows start)
    # the guard block goes into the middle: the good proofs behind it move up
    guard = [bytes([fill]) * 32] * BAD_GUARD
    b.rows = b.rows[:half] + guard + b.rows[half:]
    b.proofs = [(pos, row + BAD_GUARD if row >= half else row, e, span, uncles)
                for pos, row, e, span, uncles in b.proofs]
    zero = len(b.expected)
    b.expected.append(bytes(32))
    proofs, tops = [], []
    good = iter(zip(b.proofs, b.tops))
    for i in range(BAD_N):
        if i in BAD_AT:
            span, uncles = BAD_AT[i]
            assert half + span + uncles <= half + BAD_GUARD
            proofs.append((b.rng.getrandbits(64), half, zero if zero_expected else 0, span, uncles))
            tops.append(bytes(32))
        else:
            p, t = next(good)
            proofs.append(p)
            tops.append(t)
    b.proofs, b.tops = proofs, tops
    return b


def bad_verdicts():
    return [0 if i in BAD_AT else 1 for i in range(BAD_N)]


FAR_BASE = 1 << 27  # row 2^27 starts at byte 2^32
FAR_ROWS = FAR_BASE + 2048
FAR = ((FAR_BASE - 1, 1, 2), (FAR_BASE, 2, 64), (FAR_BASE + 600, 512, 3), (FAR_BASE + 1500, 64, 0))  # (row, span, uncles)


@functools.lru_cache(maxsize=None)
def far_proofs():
    """(block, proofs, expected, tops): block holds rows FAR_BASE - 1 .. FAR_ROWS
    - 1; only the ranges the four proofs name are meant to be written."""
    rng = random.Random(0xFA2)
    block = [rng.randbytes(32) for _ in range(FAR_ROWS - (FAR_BASE - 1))]
    proofs, tops = [], []
    for k, (row, span, uncles) in enumerate(FAR):
        assert row + span + uncles <= FAR_ROWS
        pos = rng.getrandbits(64) | (1 << 63 if uncles == 64 else 0)
        at = row - (FAR_BASE - 1)
        tops.append(walk(b"".join(block[at:at + span + uncles]), span, uncles, pos))
        proofs.append((pos, row, k, span, uncles))
    return block, proofs, list(tops), tops


def span_root(rows):
    """A span's root by the layer model (a span is a power of two: no padding)."""
    return model_root(rows, 0)
