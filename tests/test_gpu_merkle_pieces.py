"""GPU: the fused piece kernel (merkle_piece_kernel) through
device.merkle_pieces / vx_merkle_device_pieces.

The yardstick is the hashlib model below: a leaf is SHA-256 of a 16 KiB block
(the last at its real length), a slot at or past the piece's end is the zero
hash, a node is SHA-256(left || right), so an empty piece's root is the pad
hash of its height.  Everything is bit-exact, and for every shape the roots
also equal device.merkle_ragged's (leaf + node kernels) on the same buffer.
The gaps between pieces are 0xFF, so a read past a piece's end shows up as a
wrong root.  Each shape is the smallest that reaches one path of the kernel.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
KiB, MiB = 1024, 1 << 20


def sha256(b):
    return hashlib.sha256(b).digest()


def model_root(data, log2w):
    rows = [sha256(data[o:o + BLOCK]) if o < len(data) else bytes(32) for o in range(0, BLOCK << log2w, BLOCK)]
    while len(rows) > 1:
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
    return rows[0]


def pad_hash(h):
    out = bytes(32)
    for _ in range(h):
        out = sha256(out + out)
    return out


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Batch:
    """Pieces in one 0xFF-filled buffer.  offs None: in order, 16-byte aligned,
    a gap after each."""

    def __init__(self, lens, K, log2w=None, offs=None, seed=1):
        self.K = K
        self.lens = list(lens)
        self.log2w = list(log2w) if log2w is not None else None
        blob = random_bytes(seed, sum(self.lens) or 1)
        self.pieces, at = [], 0
        for ln in self.lens:
            self.pieces.append(blob[at:at + ln])
            at += ln
        if offs is None:
            offs, o = [], 0
            for ln in self.lens:
                offs.append(o)
                o += (ln + 15) // 16 * 16 + 48
        self.offs = list(offs)
        size = max([o + ln for o, ln in zip(self.offs, self.lens)] + [16])
        buf = bytearray(b"\xff" * size)
        for p, o in zip(self.pieces, self.offs):
            buf[o:o + len(p)] = p
        self.buf = buf
        self.roots = [model_root(p, self.log2w[i] if self.log2w else K) for i, p in enumerate(self.pieces)]

    def tensors(self, dev, buf=None):
        import torch

        data = torch.frombuffer(bytearray(buf if buf is not None else self.buf), dtype=torch.uint8).to(dev)
        offs = torch.tensor(self.offs, dtype=torch.int64, device=dev)
        lens = torch.tensor(self.lens, dtype=torch.int32, device=dev)
        lw = torch.tensor(self.log2w, dtype=torch.uint8, device=dev) if self.log2w is not None else None
        return data, offs, lens, lw

    def run(self, dev, expected=None, buf=None):
        """(roots of merkle_pieces, verdicts or None, roots of merkle_ragged)."""
        import torch

        from vortex_amd import device as vdev

        n = len(self.lens)
        data, offs, lens, lw = self.tensors(dev, buf)
        exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).to(dev) if expected else None
        roots = torch.full((n, 32), 0xFF, dtype=torch.uint8, device=dev)
        r, m = vdev.merkle_pieces(data, offs, lens, self.K, log2w=lw, expected=exp, roots=roots)
        r2, _, _ = vdev.merkle_ragged(data, offs, lens, self.K, log2w=lw)
        torch.cuda.synchronize()
        return r.cpu().numpy().tobytes(), (m.cpu().tolist() if m is not None else None), r2.cpu().numpy().tobytes()

    def check(self, dev):
        got, _, ragged = self.run(dev)
        for i, want in enumerate(self.roots):
            assert got[32 * i:32 * i + 32] == want, \
                f"root of piece {i} ({self.lens[i]} bytes, log2w {self.log2w[i] if self.log2w else self.K})"
        assert got == ragged, "merkle_pieces and merkle_ragged disagree"


K0_LENS = [0, 1, 55, 56, 63, 64, 65, 127, 128, 129, 16383, 16384]
K2_CYCLE = [(0, 0), (16384, 0), (16385, 1), (3 * 16384 + 1, 2), (65536, 2), (1, 0), (32768, 1), (20000, 2), (0, 2),
            (16384, 2), (16383, 1), (0, 1), (49152, 2), (129, 2)]


def shape(name):
    if name == "K0":  # two workgroups, the second partial; every tail form of a leaf
        return Batch([K0_LENS[i % len(K0_LENS)] for i in range(300)], 0)
    if name == "K2":  # 64 pieces per workgroup and a partial one; per-piece widths 0, 1, 2
        cyc = [K2_CYCLE[i % len(K2_CYCLE)] for i in range(70)]
        return Batch([c[0] for c in cyc], 2, log2w=[c[1] for c in cyc])
    if name == "K4":  # 16 pieces per workgroup: piece 16 is alone in the second
        lens = [256 * KiB, 0, 1, 16384, 16385, 100000, 256 * KiB - 1, 5 * 16384, 64, 200000, 32768, 7, 131072, 131073,
                16383, 250000, 256 * KiB - 16383]
        assert len(lens) == 17
        return Batch(lens, 4)
    if name == "K8":  # one piece per workgroup, the whole tree in LDS
        return Batch([4 * MiB, 4 * MiB - 1], 8)
    if name == "K9":  # two launches: tile tops, then the node kernel; a narrow piece beside wide ones
        return Batch([8 * MiB, 4 * MiB + 1, 3 * 16384 - 77], 9, log2w=[9, 9, 2])
    if name == "K10":
        return Batch([16 * MiB - 5], 10)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["K0", "K2", "K4", "K8", "K9", "K10"])
def test_roots_equal_the_model_and_the_leaf_node_pair(built, gpu, name):
    shape(name).check(gpu)


def test_empty_piece_is_the_pad_hash(built, gpu):
    b = Batch([0, 0, 0, 16384], 3, log2w=[0, 1, 3, 3])
    assert b.roots[:3] == [pad_hash(0), pad_hash(1), pad_hash(3)]
    b.check(gpu)


def test_offsets_not_256_aligned_and_pieces_in_reverse_order(built, gpu):
    """Piece i lies before piece i-1 in the buffer, at offsets that are
    multiples of 16 and of nothing larger."""
    lens = [65536, 16385, 40000, 0, 65535]
    offs, o = [0] * len(lens), 16
    for i in reversed(range(len(lens))):
        offs[i] = o
        o += (lens[i] + 15) // 16 * 16 + 16
        if (o // 16) % 2 == 0:
            o += 16
    assert all(x % 16 == 0 and x % 32 == 16 for x in offs) and offs == sorted(offs, reverse=True)
    Batch(lens, 2, offs=offs, seed=5).check(gpu)


def test_verdicts_against_one_flipped_byte(built, gpu):
    b = Batch([65536, 65536, 16385, 0, 65535, 40000], 2, seed=7)
    flipped = bytearray(b.buf)
    flipped[b.offs[0] + 65535] ^= 0x10  # piece 0's last leaf
    got, matched, ragged = b.run(gpu, expected=b.roots, buf=flipped)
    assert matched == [0, 1, 1, 1, 1, 1]
    assert got == ragged and got[32:] == b"".join(b.roots[1:]) and got[:32] != b.roots[0]
    _, clean, _ = b.run(gpu, expected=b.roots)
    assert clean == [1] * 6


def test_verdicts_on_the_two_launch_path(built, gpu):
    """Above 256 leaves the node kernel emits the verdicts, narrow pieces included."""
    b = shape("K9")
    exp = list(b.roots)
    exp[1] = bytes(32)
    _, matched, _ = b.run(gpu, expected=exp)
    assert matched == [1, 0, 1]


def test_no_pieces_launches_nothing(built, gpu):
    import torch

    from vortex_amd import device as vdev

    data = torch.zeros(16, dtype=torch.uint8, device=gpu)
    empty64 = torch.empty(0, dtype=torch.int64, device=gpu)
    empty32 = torch.empty(0, dtype=torch.int32, device=gpu)
    for K in (0, 3, 9):
        roots, matched = vdev.merkle_pieces(data, empty64, empty32, K)
        assert roots.shape == (0, 32) and matched is None
    torch.cuda.synchronize()


def test_layout_checks_before_launch(built, gpu):
    """The checks of merkle_ragged, under this entry's name."""
    import torch

    from vortex_amd import device as vdev

    data = torch.zeros(65536, dtype=torch.uint8, device=gpu)

    def call(offs, lens, K, lw=None):
        return vdev.merkle_pieces(data, torch.tensor(offs, dtype=torch.int64, device=gpu),
                                  torch.tensor(lens, dtype=torch.int32, device=gpu), K,
                                  log2w=torch.tensor(lw, dtype=torch.uint8, device=gpu) if lw else None)

    with pytest.raises(ValueError, match="merkle_pieces: every offset"):
        call([8], [16], 0)
    with pytest.raises(ValueError, match="past the data tensor"):
        call([65520], [17], 0)
    with pytest.raises(ValueError, match="longer than its tree"):
        call([0], [16385], 0)
    with pytest.raises(ValueError, match="log2w 3 > log2_width 2"):
        call([0], [16], 2, lw=[3])
    torch.cuda.synchronize()
