"""GPU: the SHA-256 merkle kernels at the edges the other merkle tests leave out.

  * leaf lengths 128 g + r around the leaf kernels' two-group ring, twelve
    tails at seven group counts, each group count a wave of its own; every
    tail 0..127, waves that mix group counts and each of the five entries of
    the leaf lane on its own are in test_gpu_merkle_leaf_sweep.py;
  * per-piece widths (log2w) under a batch wider than one node tile
    (log2_width = 10, the smallest such width; widths 11 to 17, where the
    wide kernels have more than two tiles per piece, are in
    test_gpu_merkle_wide.py);
  * verdicts against an expected root that is one bit off, a different byte
    for every piece: so far a mismatch was a flipped data byte or a zero row;
  * pieces at offsets at or above 4 GiB.

The yardstick is hashlib.sha256 and the BEP 52 model below; everything is
bit-exact.  As in test_gpu_merkle.py the gaps between pieces and every output
tensor are 0xFF before each call, so a read past a piece's end or an unwritten
row shows up as a mismatch; output tensors have one spare row that must stay
0xFF.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
LEAF_GROUPS = (0, 1, 2, 3, 4, 5, 127)
LEAF_TAILS = (0, 1, 3, 4, 55, 56, 63, 64, 65, 119, 120, 127)
LEAF_LENGTHS = [128 * g + r for g in LEAF_GROUPS for r in LEAF_TAILS if 128 * g + r <= BLOCK]


def sha256(b):
    return hashlib.sha256(b).digest()


def leaf_rows(data, log2_width):
    return [sha256(data[o:o + BLOCK]) if o < len(data) else bytes(32) for o in range(0, BLOCK << log2_width, BLOCK)]


def tree_root(rows):
    while len(rows) > 1:
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
    return rows[0]


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def one_bit_off(roots):
    """Piece i's root with one bit of byte i % 32 flipped."""
    out = []
    for i, r in enumerate(roots):
        b = bytearray(r)
        b[i % 32] ^= 1 << ((i // 4) % 8)
        out.append(bytes(b))
    return out


class Batch:
    """Pieces in one 0xFF-filled buffer at 16-byte aligned offsets, a gap of 48
    bytes after each, and what BEP 52 says about them."""

    def __init__(self, pieces, log2_width, log2w=None):
        self.pieces, self.K = pieces, log2_width
        self.log2w = list(log2w) if log2w is not None else None
        self.offs, o = [], 0
        for p in pieces:
            self.offs.append(o)
            o += (len(p) + 15) // 16 * 16 + 48
        buf = bytearray(b"\xff" * max(o, 16))
        for p, off in zip(pieces, self.offs):
            buf[off:off + len(p)] = p
        self.buf = buf
        self.leaves = [leaf_rows(p, log2_width) for p in pieces]
        self.roots = [tree_root(rows[:1 << (self.log2w[i] if self.log2w else log2_width)])
                      for i, rows in enumerate(self.leaves)]

    def tensors(self, dev):
        import torch

        return (torch.frombuffer(self.buf, dtype=torch.uint8).to(dev),
                torch.tensor(self.offs, dtype=torch.int64, device=dev),
                torch.tensor([len(p) for p in self.pieces], dtype=torch.int32, device=dev),
                torch.tensor(self.log2w, dtype=torch.uint8, device=dev) if self.log2w is not None else None)

    def check_roots(self, got, who):
        n = len(self.pieces)
        for i, want in enumerate(self.roots):
            assert got[32 * i:32 * i + 32] == want, \
                f"{who}: root of piece {i} ({len(self.pieces[i])} bytes, log2w {self.log2w[i] if self.log2w else self.K})"
        assert got[32 * n:] == b"\xff" * 32, f"{who}: the spare root row was written"

    def ragged(self, dev, expected=None, check_leaves=True):
        """merkle_ragged: roots and leaf rows checked; returns the verdicts."""
        import torch

        from vortex_amd import device as vdev

        n = len(self.pieces)
        data, offs, lens, lw = self.tensors(dev)
        leaves = torch.full(((n << self.K) + 1, 32), 0xFF, dtype=torch.uint8, device=dev)
        roots = torch.full((n + 1, 32), 0xFF, dtype=torch.uint8, device=dev)
        matched = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device=dev)
        exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).to(dev) if expected else None
        vdev.merkle_ragged(data, offs, lens, self.K, log2w=lw, expected=exp, leaves=leaves, roots=roots,
                           matched=matched if expected else None)
        torch.cuda.synchronize()
        self.check_roots(roots.cpu().numpy().tobytes(), "merkle_ragged")
        if check_leaves:
            got = leaves.cpu().numpy().tobytes()
            want = b"".join(b"".join(rows) for rows in self.leaves)
            if got[:len(want)] != want:
                w = 1 << self.K
                bad = [k for k in range(n << self.K) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
                raise AssertionError(f"merkle_ragged: {len(bad)} leaf rows differ, first: piece {bad[0] // w} "
                                     f"({len(self.pieces[bad[0] // w])} bytes) slot {bad[0] % w}")
            assert got[len(want):] == b"\xff" * 32, "merkle_ragged: the spare leaf row was written"
        m = matched.cpu().tolist()
        assert m[n] == 0xFF
        return m[:n] if expected else None

    def fused(self, dev, expected=None):
        """merkle_pieces: roots checked; returns the verdicts."""
        import torch

        from vortex_amd import device as vdev

        n = len(self.pieces)
        data, offs, lens, lw = self.tensors(dev)
        roots = torch.full((n + 1, 32), 0xFF, dtype=torch.uint8, device=dev)
        matched = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device=dev)
        exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).to(dev) if expected else None
        vdev.merkle_pieces(data, offs, lens, self.K, log2w=lw, expected=exp, roots=roots,
                           matched=matched if expected else None)
        torch.cuda.synchronize()
        self.check_roots(roots.cpu().numpy().tobytes(), "merkle_pieces")
        m = matched.cpu().tolist()
        assert m[n] == 0xFF
        return m[:n] if expected else None


def _waves_of_leaf_lengths():
    """Every leaf length, each group count g as a wave of its own (its twelve
    tails repeated to 64 lanes), so the wave-wide ring bound is g itself."""
    return [128 * g + LEAF_TAILS[k % len(LEAF_TAILS)] for g in LEAF_GROUPS for k in range(64)]


def test_leaf_lengths_as_whole_pieces(built, gpu):
    """log2_width = 0: the root is the SHA-256 of the piece."""
    assert len(LEAF_LENGTHS) == 84 and max(LEAF_LENGTHS) == BLOCK - 1
    lens = _waves_of_leaf_lengths()
    blob = random_bytes(1, sum(lens))
    pieces, at = [], 0
    for L in lens:
        pieces.append(blob[at:at + L])
        at += L
    b = Batch(pieces, 0)
    assert b.roots == [sha256(p) if p else bytes(32) for p in pieces]  # an empty piece: the zero hash
    assert b.ragged(gpu, expected=b.roots) == [1] * len(lens)
    assert b.fused(gpu, expected=b.roots) == [1] * len(lens)


def test_leaf_lengths_as_the_last_leaf_of_four(built, gpu):
    """Three full leaves and a fourth of every length (0: the zero hash)."""
    pieces = [random_bytes(100 + L, 3 * BLOCK + L) for L in LEAF_LENGTHS]
    b = Batch(pieces, 2)
    exp = one_bit_off(b.roots)
    assert b.ragged(gpu, expected=exp) == [0] * len(pieces)
    assert b.fused(gpu, expected=b.roots) == [1] * len(pieces)


def test_leaf_lengths_as_stage_blocks(built, gpu):
    """merkle_blocks: block b of the stage holds lens[b] bytes, the rest of
    its 16 KiB is 0xFF; rows in reverse order, one row skipped."""
    import torch

    from vortex_amd import device as vdev

    lens = _waves_of_leaf_lengths()
    n = len(lens)
    stage = bytearray(b"\xff" * (n * BLOCK))
    want = []
    for k, L in enumerate(lens):
        body = random_bytes(5000 + k, L)
        stage[k * BLOCK:k * BLOCK + L] = body
        want.append(sha256(body) if L else bytes(32))  # an absent slot: the zero hash
    rows = [n - 1 - k for k in range(n)]
    skipped = 70
    rows[skipped] = vdev.SKIP_ROW
    leaves = torch.full((n + 1, 32), 0xFF, dtype=torch.uint8, device=gpu)
    vdev.merkle_blocks(torch.frombuffer(stage, dtype=torch.uint8).to(gpu),
                       torch.tensor(rows, dtype=torch.int64, device=gpu),
                       torch.tensor(lens, dtype=torch.int32, device=gpu), leaves)
    torch.cuda.synchronize()
    got = leaves.cpu().numpy().tobytes()
    for k, L in enumerate(lens):
        r = n - 1 - k
        assert got[32 * r:32 * r + 32] == (want[k] if k != skipped else b"\xff" * 32), f"block {k} ({L} bytes)"
    assert got[32 * n:] == b"\xff" * 32


WIDE = [  # (length, log2w): one piece of each width under log2_width = 10
    (1000, 0), (BLOCK + 100, 1), (3 * (1 << 20) + BLOCK + 1, 8), (5 * (1 << 20) + 77, 9), ((16 << 20) - 5, 10),
    (BLOCK, 0), (2 * BLOCK, 1), (4 << 20, 8), (8 << 20, 9),  # full trees: no short last leaf
]


def test_per_piece_widths_under_a_wide_batch(built, gpu):
    """merkle_ragged: the wide node kernel's early exit (log2w <= one tile) and
    its reduction of the tiles' tops, with log2w set; merkle_pieces: tiles
    under the piece's own root only (want_top 0, 1, 2)."""
    pieces = [random_bytes(7000 + i, L) for i, (L, _) in enumerate(WIDE)]
    b = Batch(pieces, 10, log2w=[w for _, w in WIDE])
    assert b.roots[0] == sha256(pieces[0]) and b.roots[5] == sha256(pieces[5])
    exp = one_bit_off(b.roots)
    for k in (2, 4, 5):
        exp[k] = b.roots[k]
    verdicts = [int(k in (2, 4, 5)) for k in range(len(WIDE))]
    assert b.ragged(gpu, expected=exp) == verdicts
    assert b.fused(gpu, expected=exp) == verdicts
    assert b.ragged(gpu, expected=b.roots, check_leaves=False) == [1] * len(WIDE)
    assert b.fused(gpu, expected=b.roots) == [1] * len(WIDE)


@pytest.mark.parametrize("entry,log2_width", [("ragged", 2), ("ragged", 10), ("pieces", 2), ("pieces", 9)])
def test_verdict_needs_every_word_of_the_root(built, gpu, entry, log2_width):
    """64 pieces; the expected root of piece i is one bit away from the true
    one in byte i % 32, so every word of the compare decides two verdicts."""
    n = 64
    lens = [min(BLOCK << log2_width, (i % 4) * BLOCK + 1 + 251 * i) for i in range(n)]
    b = Batch([random_bytes(9000 + i, L) for i, L in enumerate(lens)], log2_width)
    run = b.ragged if entry == "ragged" else b.fused
    assert run(gpu, expected=one_bit_off(b.roots)) == [0] * n
    assert run(gpu, expected=b.roots) == [1] * n


def test_offsets_at_and_above_4_gib(built, gpu):
    """Two short pieces behind the 4 GiB line of one tensor (never filled:
    only the pieces and the bytes around them are written)."""
    import torch

    from vortex_amd import device as vdev

    base = 1 << 32
    data = torch.empty(base + (1 << 20), dtype=torch.uint8, device=gpu)
    offs = [base + 16, base + 65536]
    pieces = [random_bytes(31, 40007), random_bytes(32, BLOCK + 129)]
    data[base:base + 131072] = 0xFF
    for o, p in zip(offs, pieces):
        data[o:o + len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(gpu)
    d_offs = torch.tensor(offs, dtype=torch.int64, device=gpu)
    d_lens = torch.tensor([len(p) for p in pieces], dtype=torch.int32, device=gpu)
    sha1_want = b"".join(hashlib.sha1(p).digest() for p in pieces)
    for variant in (0, 1):
        dig = torch.full((3, 20), 0xA5, dtype=torch.uint8, device=gpu)
        vdev.sha1_ragged(data, d_offs, d_lens, digests=dig, variant=variant)
        torch.cuda.synchronize()
        assert dig.cpu().numpy().tobytes() == sha1_want + b"\xa5" * 20, f"sha1_ragged variant {variant}"
    want = [tree_root(leaf_rows(p, 2)) for p in pieces]
    exp = torch.frombuffer(bytearray(want[0] + one_bit_off(want)[1]), dtype=torch.uint8).to(gpu)
    roots, leaves, matched = vdev.merkle_ragged(data, d_offs, d_lens, 2, expected=exp)
    roots2, matched2 = vdev.merkle_pieces(data, d_offs, d_lens, 2, expected=exp)
    torch.cuda.synchronize()
    assert roots.cpu().numpy().tobytes() == b"".join(want) == roots2.cpu().numpy().tobytes()
    assert leaves.cpu().numpy().tobytes() == b"".join(b"".join(leaf_rows(p, 2)) for p in pieces)
    assert matched.cpu().tolist() == [1, 0] == matched2.cpu().tolist()
