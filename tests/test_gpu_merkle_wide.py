"""GPU: BitTorrent v2 merkle trees wider than 1,024 leaves (pieces above 16 MiB).

Every v2 entry takes trees of up to 2^17 leaf slots (a 2 GiB piece); the other
merkle tests stop at log2_width 10, where most of the wide code is degenerate:
two tile tops and one top level in merkle_wide_node_kernel, tshift 1 and 2 in
merkle_piece_kernel, 8 bitmap words per piece in merkle_block_check_kernel.
Here:

  * the node kernels alone at widths 10..17 over random rows (every tile top
    distinct), one piece per log2w of {0, 8, 9, 10, 11, W - 1, W};
  * leaf + node and the fused piece kernel at widths 11..17: full 32 MiB and
    64 MiB pieces, and sparse batches (a few MiB of data in trees of up to
    2^17 slots: whole workgroups of absent slots) with per-piece widths under
    the batch's;
  * the block check at 32 and 2,048 bitmap words per piece;
  * the hybrid device call and every context path at 32 MiB pieces.

The yardstick is hashlib through the model of test_gpu_merkle_edges.py
(leaf_rows / tree_root) and its conventions: pieces in one 0xFF-filled buffer
at 16-byte aligned offsets with a 48-byte gap, every output tensor 0xFF before
the call with one spare row or word that must stay 0xFF.  Everything is
bit-exact.  No 2 GiB piece is built: the widest trees are sparse.
"""
import ctypes
import functools
import hashlib
import os
import random
import time

import pytest

from test_gpu_merkle_async import collect
from test_gpu_merkle_edges import BLOCK, Batch, leaf_rows, one_bit_off, random_bytes, sha256, tree_root

pytestmark = pytest.mark.gpu

MiB = 1 << 20
FF64 = 0xFFFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=None)
def data(seed, n):
    """random_bytes, made once per (seed, length) and shared."""
    return random_bytes(seed, n)


def table(rows, dev):
    import torch

    return torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev)


# ---- 1a. the node kernels alone ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def node_case(W):
    """(log2w per piece, the leaf rows of all pieces, the roots): one piece per
    width of {0, 8, 9, 10, 11, W - 1, W} that the batch width allows, the
    widest not first.  Rows past a piece's 2^log2w stay random."""
    widths = sorted({w for w in (0, 8, 9, 10, 11, W - 1, W) if w <= W})
    random.Random(4242 + W).shuffle(widths)
    if widths[0] == W:
        widths.append(widths.pop(0))
    rows = random.Random(W).randbytes(len(widths) << W << 5)
    roots = []
    for i, w in enumerate(widths):
        at = (i << W) * 32
        roots.append(tree_root([rows[at + 32 * k:at + 32 * k + 32] for k in range(1 << w)]))
    return widths, rows, roots


def run_nodes(dev, rows, n, W, log2w, expected=None):
    """merkle_nodes into 0xFF-filled outputs of one spare row: (root rows, verdicts)."""
    import torch

    from vortex_amd import device as vdev

    leaves = torch.frombuffer(bytearray(rows), dtype=torch.uint8).to(dev)
    roots = torch.full((n + 1, 32), 0xFF, dtype=torch.uint8, device=dev)
    matched = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device=dev)
    lw = torch.tensor(log2w, dtype=torch.uint8, device=dev) if log2w is not None else None
    got_roots, got_matched = vdev.merkle_nodes(leaves, n, W, log2w=lw,
                                               expected=table(expected, dev) if expected else None, roots=roots,
                                               matched=matched if expected else None)
    torch.cuda.synchronize()
    assert got_roots is roots and (got_matched is matched if expected else got_matched is None)
    assert leaves.cpu().numpy().tobytes() == rows, "the leaf rows were written"
    raw, m = roots.cpu().numpy().tobytes(), matched.cpu().tolist()
    assert raw[32 * n:] == b"\xff" * 32, "the spare root row was written"
    assert m[n] == 0xFF and (expected or m == [0xFF] * (n + 1))
    return [raw[32 * i:32 * i + 32] for i in range(n)], m[:n]


@pytest.mark.parametrize("W", range(10, 18))
def test_nodes_one_piece_per_width(built, gpu, W):
    """Above width 9 every piece is a workgroup of merkle_wide_node_kernel: 1 to
    256 tiles, their tops reduced over 0 to 8 levels, the root taken from the
    first tile (log2w <= 9) or from the tops."""
    widths, rows, want = node_case(W)
    n = len(widths)
    assert n == (4 if W == 10 else 5 if W == 11 else 6 if W == 12 else 7) and widths[0] != W and W in widths
    got, _ = run_nodes(gpu, rows, n, W, widths)
    assert [i for i in range(n) if got[i] != want[i]] == [], (widths, "pieces whose root differs")
    # verdicts: every expected root one bit off, but the widest piece's
    true = widths.index(W)
    exp = one_bit_off(want)
    exp[true] = want[true]
    got, m = run_nodes(gpu, rows, n, W, widths, expected=exp)
    assert got == want and m == [int(i == true) for i in range(n)]


@pytest.mark.parametrize("W", range(10, 18))
def test_nodes_two_full_pieces_without_log2w(built, gpu, W):
    _, rows, _ = node_case(W)
    rows = rows[:2 << W << 5]
    want = [tree_root([rows[32 * k:32 * k + 32] for k in range(i << W, (i + 1) << W)]) for i in range(2)]
    exp = [want[0], one_bit_off(want)[1]]
    got, m = run_nodes(gpu, rows, 2, W, None, expected=exp)
    assert got == want and m == [1, 0]
    got, _ = run_nodes(gpu, rows, 2, W, None)
    assert got == want


# ---- 1b. leaf + node, and the fused piece kernel ----------------------------------

class WideBatch(Batch):
    """Batch, with its tensors uploaded once and the roots of the last call of
    each entry kept, so the two entries can be compared with each other."""

    def __init__(self, pieces, log2_width, log2w=None):
        super().__init__(pieces, log2_width, log2w)
        self.seen, self._dev = {}, None

    def tensors(self, dev):
        if self._dev is None:
            self._dev = super().tensors(dev)
        return self._dev

    def check_roots(self, got, who):
        super().check_roots(got, who)
        self.seen[who] = got

    def both(self, dev, off):
        """merkle_ragged (roots, the whole leaf layer, verdicts) and
        merkle_pieces (roots, verdicts) against the model and each other; the
        expected root of piece `off` is one bit off."""
        n = len(self.pieces)
        exp = list(self.roots)
        exp[off] = one_bit_off(self.roots)[off]
        want = [int(i != off) for i in range(n)]
        assert self.ragged(dev, expected=exp) == want
        assert self.fused(dev, expected=exp) == want
        assert self.seen["merkle_ragged"] == self.seen["merkle_pieces"]
        assert self._dev[0].cpu().numpy().tobytes() == bytes(self.buf), "the data was written"


SPARSE_LENS = (257 * BLOCK + 77,           # crosses a 256-leaf tile of the fused kernel
               1,
               (3 * 512 + 2) * BLOCK + 129)  # four node tiles with distinct tops, the rest zero-hash tiles
SPARSE_NARROW = (9, 0, 11)                 # the pieces' own widths: narrow, one leaf, mid-width


@functools.lru_cache(maxsize=None)
def sparse(W, narrow):
    pieces = [data(300 + i, L) for i, L in enumerate(SPARSE_LENS)]
    return WideBatch(pieces, W, log2w=SPARSE_NARROW if narrow else (W,) * 3)


@pytest.mark.parametrize("W,lens,off", [(11, (32 * MiB, 16 * MiB + BLOCK + 5), 0), (12, (64 * MiB - 5,), 0)],
                         ids=["32MiB-x2", "64MiB-5"])
def test_full_pieces(built, gpu, W, lens, off):
    """Real bytes in every tile: 8 and 16 fused tiles and 4 and 8 node tiles
    per piece, all different; at width 11 a second piece behind the first,
    half empty under the full width."""
    b = WideBatch([data(200 + 10 * W + i, L) for i, L in enumerate(lens)], W, log2w=(W,) * len(lens))
    b.both(gpu, off)
    if len(lens) > 1:
        b.both(gpu, len(lens) - 1)


@pytest.mark.parametrize("narrow", [False, True], ids=["log2w=W", "log2w=9,0,11"])
@pytest.mark.parametrize("W", [13, 15, 17])
def test_sparse_pieces(built, gpu, W, narrow):
    """Three pieces of 4 MiB, 1 byte and 24 MiB in trees of 2^W slots: slot
    starts up to 2^31 - 16 KiB, thousands of consecutive waves of absent
    slots, tshift 5, 7 and 9 with a second and a third piece.  With the
    pieces' own widths 9, 0 and 11 the fused kernel stores 2, 1 and 8 of each
    piece's 2^tshift tops (want_top < tshift) and the node kernels stop below
    the batch width."""
    b = sparse(W, narrow)
    if narrow:
        assert b.roots[1] == sha256(b.pieces[1]) and b.roots != sparse(W, False).roots
    b.both(gpu, 2)
    b.both(gpu, 0)


def test_longer_than_its_own_tree_is_refused_before_launch(built, gpu):
    """As test_gpu_merkle_pieces.py::test_layout_checks_before_launch, at wide
    widths: a piece one byte longer than 16384 << log2w[i], alone or behind a
    good piece, with its own width or the batch's."""
    import torch

    from vortex_amd import device as vdev

    buf = torch.empty((BLOCK << 11) + 64, dtype=torch.uint8, device=gpu)
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=gpu)  # noqa: E731
    cases = [([0], [(BLOCK << 11) + 1], 11, None),
             ([0], [(BLOCK << 9) + 1], 13, [9]),
             ([0, 16], [1, (BLOCK << 10) + 1], 17, [17, 10]),
             ([0], [(BLOCK << 11) + 1], 17, [11])]
    for offs, lens, W, lw in cases:
        n = len(offs)
        roots = torch.full((n, 32), 0xFF, dtype=torch.uint8, device=gpu)
        for entry in (vdev.merkle_ragged, vdev.merkle_pieces):
            with pytest.raises(ValueError, match="longer than its tree"):
                entry(buf, t(offs, torch.int64), t(lens, torch.int32), W,
                      log2w=t(lw, torch.uint8) if lw else None, roots=roots)
        torch.cuda.synchronize()
        assert bool((roots == 0xFF).all()), "a refused call launched"
    with pytest.raises(ValueError, match="longer than its tree"):
        vdev.merkle_block_check(buf, t([0], torch.int64), t([(BLOCK << 11) + 1], torch.int32), 11)
    # lens is int32: the bits of 2^31, the one length above it that the C ABI's uint32 allows
    with pytest.raises(ValueError, match="2\\^31"):
        vdev.merkle_pieces(buf, t([0], torch.int64), t([-1 << 31], torch.int32), 17)


# ---- 1c. the block check ----------------------------------------------------------

def run_block_check(dev, b, W, buf, exp_rows, want_leaves):
    """One call over batch b's layout with 0xFF-filled outputs of one spare
    word / row: (bitmap words, leaf bytes or None)."""
    import torch

    from vortex_amd import device as vdev

    n = len(b.pieces)
    wpp = (1 << W) // 64
    bad = torch.full((n * wpp + 1,), -1, dtype=torch.int64, device=dev) if exp_rows is not None else None
    leaves = torch.full(((n << W) + 1, 32), 0xFF, dtype=torch.uint8, device=dev) if want_leaves else None
    exp = torch.frombuffer(bytearray(exp_rows), dtype=torch.uint8).to(dev) if exp_rows is not None else None
    got_bad, got_leaves = vdev.merkle_block_check(
        torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev),
        torch.tensor(b.offs, dtype=torch.int64, device=dev),
        torch.tensor([len(p) for p in b.pieces], dtype=torch.int32, device=dev), W, expected_leaves=exp,
        leaves=leaves, bad=bad, want_leaves=want_leaves)
    torch.cuda.synchronize()
    assert got_bad is bad and got_leaves is leaves
    words = raw = None
    if bad is not None:
        words = bad.cpu().numpy().view("uint64").tolist()
        assert words.pop() == FF64, "the word past the bitmap was written"
    if leaves is not None:
        raw = leaves.cpu().numpy().tobytes()
        assert raw[32 * (n << W):] == b"\xff" * 32, "the row past the leaves was written"
        raw = raw[:32 * (n << W)]
    return words, raw


@pytest.mark.parametrize("W", [11, 17])
def test_block_check_32_and_2048_words_per_piece(built, gpu, W):
    b = sparse(W, False)
    n, wpp = 3, (1 << W) // 64
    good = b"".join(b"".join(rows) for rows in b.leaves)
    # the good rows, with garbage in every slot at or past its piece's end: those are never bad
    exp = bytearray(random.Random(0xB10C + W).randbytes(len(good)))
    nblocks = [-(-len(p) // BLOCK) for p in b.pieces]
    for i, k in enumerate(nblocks):
        at = (i << W) * 32
        exp[at:at + 32 * k] = good[at:at + 32 * k]
    assert nblocks == [258, 1, 1539]
    words, raw = run_block_check(gpu, b, W, b.buf, exp, True)
    assert words == [0] * (n * wpp) and raw == good
    # blocks 0, 63, 64 and the last (short) block of piece 0; the last block of piece 2
    hits = {0: [0, 63, 64, 257], 2: [1538]}
    buf = bytearray(b.buf)
    for i, blocks in hits.items():
        for k in blocks:
            buf[b.offs[i] + min(k * BLOCK + 5 * k, len(b.pieces[i]) - 1)] ^= 0x20
    want = [0] * (n * wpp)
    for i, blocks in hits.items():
        for k in blocks:
            want[i * wpp + (k >> 6)] |= 1 << (k & 63)
    assert want[0] == 1 | 1 << 63 and want[1] == 1 and want[4] == 2 and want[2 * wpp + 24] == 4
    words, none = run_block_check(gpu, b, W, buf, exp, False)
    assert none is None
    assert [(k, hex(w)) for k, w in enumerate(words) if w != want[k]] == []
    if W == 17:  # the leaves-only form
        none, raw = run_block_check(gpu, b, W, b.buf, None, True)
        assert none is None and raw == good


# ---- 1d. the hybrid device call ---------------------------------------------------

def test_hybrid_device_call_at_32_mib(built, gpu):
    """Four pieces at log2_width 11: full; half a piece and a bit, padded;
    one byte and 524,287 zero blocks of pad behind its block; 119 bytes, the
    torrent's last.  log2w alternates between the full width and the piece's own."""
    from test_gpu_hybrid import reference, run_device

    pl = 32 * MiB
    shapes = [(pl, 0), (16 * MiB + BLOCK + 5, pl - (16 * MiB + BLOCK + 5)), (1, pl - 1), (119, 0)]
    pieces, lw, want1, want2 = reference(pl, shapes, 11)
    assert lw == [11, 11, 11, 0]
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw, want1, want2)
    assert [i for i in range(4) if got1[i] != want1[i]] == [], "SHA-1"
    assert [i for i in range(4) if got2[i] != want2[i]] == [], "roots"
    assert m == [3] * 4
    # one wrong row of each table, in different pieces: each clears its own bit only
    e1, e2 = list(want1), list(want2)
    e1[2] = hashlib.sha1(want1[2]).digest()
    e2[1] = hashlib.sha256(want2[1]).digest()
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw, e1, e2)
    assert (got1, got2, m) == (want1, want2, [3, 1, 2, 3])


# ---- 2. the context paths at 32 MiB pieces ----------------------------------------

PL = 32 * MiB
FLENS = [PL + 12345, 3 * BLOCK + 5]  # a.bin: a full piece and a short one at width 11; b.bin: one piece of width 2


@pytest.fixture(scope="module")
def pool(built, gpu):
    from vortex_amd.hash_pool import HashPool

    p = HashPool(PL, slots=3, batch_pieces=8, slot_bytes=64 * MiB)
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def three_pieces():
    """(pieces, log2w, leaf rows, roots): a full piece, the short last piece of
    a long file, and a 5-byte file's piece at its own width."""
    pieces = [data(400, FLENS[0])[:PL], data(401, PL // 3 + 17), data(402, 5)]
    lw = [11, 11, 0]
    leaves = [leaf_rows(p, w) for p, w in zip(pieces, lw)]
    return pieces, lw, leaves, [tree_root(rows) for rows in leaves]


@functools.lru_cache(maxsize=None)
def torrent():
    """(file bytes, the pieces' bytes, pads, log2w, v1 digests, v2 rows) of FLENS as a hybrid torrent."""
    from vortex_amd import hybrid

    files = [data(400 + k, n) for k, n in enumerate(FLENS)]
    findex, foff, dlen, pads, lw = hybrid.hybrid_pieces(FLENS, PL)
    parts = [files[f][o:o + d] for f, o, d in zip(findex, foff, dlen)]
    assert [len(p) for p in parts] == [PL, 12345, 3 * BLOCK + 5] and pads == [0, PL - 12345, 0] and lw == [11, 11, 2]
    return (files, parts, pads, lw, [hybrid.v1_digest(p, pad) for p, pad in zip(parts, pads)],
            [hybrid.v2_root(p, w) for p, w in zip(parts, lw)])


def write_files(tmp_path):
    paths = []
    for name, body in zip(("a.bin", "b.bin"), torrent()[0]):
        paths.append(os.path.join(str(tmp_path), name))
        with open(paths[-1], "wb") as f:
            f.write(body)
    return paths


def test_verify_merkle_at_32_mib(pool):
    pieces, lw, _, roots = three_pieces()
    exp = list(roots)
    exp[1] = one_bit_off(roots)[1]
    assert pool.verify_merkle(pieces, exp, PL, log2w=lw) == ([True, False, True], roots)
    assert pool.verify_merkle(pieces[:2], roots[:2], PL) == ([True, True], roots[:2])  # the default width


def test_spawn_merkle_at_32_mib(pool):
    """One slot of three pieces at kmax 11: the fused kernel's 8 tiles per
    piece, then the node launch over the tops."""
    pieces, lw, _, roots = three_pieces()
    exp = list(roots)
    exp[0] = one_bit_off(roots)[0]
    batches = pool.stats()["batches"]
    for i, (p, w) in enumerate(zip(pieces, lw)):
        pool.spawn_merkle(i, 5, p, len(p), exp[i], log2w=w)
    assert pool.pending == 3
    pool.flush()
    got = collect(pool, 3)
    assert sorted((r.index, r.conn_id, r.hash_matched, r.digest) for r in got) == \
        [(i, 5, i != 0, roots[i]) for i in range(3)]
    assert pool.pending == 0 and pool.try_recv_merkle() is None and pool.try_iter() == []
    assert pool.stats()["batches"] == batches + 1


def test_check_blocks_at_32_words_per_piece(pool):
    from vortex_amd.hash_pool import _ptr_arrays

    pieces, _, leaves, _ = three_pieces()
    hits = [[5, 1999], [682]]  # words 0 and 31 of piece 0; the short last block of piece 1, word 10
    good = [b"".join(leaves[i]) for i in range(2)]
    bufs, now = [], []
    for i in range(2):
        p, rows = bytearray(pieces[i]), list(leaves[i])
        for k in hits[i]:
            p[min(k * BLOCK + 3 * k, len(p) - 1)] ^= 0x01
            rows[k] = sha256(bytes(p[k * BLOCK:(k + 1) * BLOCK]))
        assert rows[hits[i][-1]] != leaves[i][hits[i][-1]]
        bufs.append(p)
        now.append(b"".join(rows))
    assert len(pieces[1]) == 682 * BLOCK + 10939
    before = pool.stats()
    assert pool.check_blocks(bufs, PL, good, want_leaves=True) == (hits, now)
    assert pool.check_blocks(bufs, PL, now) == ([[], []], None)
    # the C call's own bitmap and counts, 0xFF-filled first, one spare entry each
    ptrs, lens, keep = _ptr_arrays(bufs)
    exp = ctypes.create_string_buffer(b"".join(good), 2 * 2048 * 32)
    words = (ctypes.c_uint64 * 65)(*[FF64] * 65)
    counts = (ctypes.c_uint32 * 3)(*[0xFFFFFFFF] * 3)
    assert pool.lib.vx_merkle_check_blocks(pool._h, ptrs, lens, 2, PL, exp, words, counts, None) == 0
    want = [0] * 64 + [FF64]
    for i in range(2):
        for k in hits[i]:
            want[32 * i + (k >> 6)] |= 1 << (k & 63)
    assert list(words) == want and want[31] == 1 << (1999 & 63) and want[32 + 10] == 1 << (682 & 63)
    assert list(counts) == [2, 1, 0xFFFFFFFF]
    assert pool.stats() == before and pool.pending == 0
    del keep


def test_files_verify_and_hash_at_32_mib(pool, tmp_path):
    from vortex_amd import merkle

    _, _, _, _, _, rows = torrent()
    paths = write_files(tmp_path)
    io0 = pool.stats()["io_errors"]
    assert pool.verify_merkle_files(paths, FLENS, PL, b"".join(rows)) == ([True] * 3, 0)
    assert pool.last_verify()["read_bytes"] == sum(FLENS)
    got_rows, ok, tree, bad = pool.hash_merkle_files(paths, FLENS, PL)
    assert (got_rows, ok, bad) == (b"".join(rows), [True] * 3, 0)
    assert merkle.tree_layout(FLENS, PL) == ([2, 1], [0, 3, 4])
    assert tree == merkle.build_tree(rows[:2], 11) + rows[2], "the files' trees differ from hashlib"
    # one byte of a.bin's second piece
    with open(paths[0], "r+b") as f:
        f.seek(PL + 100)
        f.write(bytes([torrent()[0][0][PL + 100] ^ 0x40]))
    assert pool.verify_merkle_files(paths, FLENS, PL, b"".join(rows)) == ([True, False, True], 0)
    assert pool.stats()["io_errors"] == io0


def test_verify_hybrid_files_at_32_mib(pool, tmp_path):
    """The second piece is 12,345 bytes and 32 MiB - 12,345 zeros that exist nowhere."""
    _, _, _, _, v1, rows = torrent()
    paths = write_files(tmp_path)
    assert pool.verify_hybrid_files(paths, FLENS, PL, b"".join(v1), b"".join(rows)) == [(True, True)] * 3
    assert pool.last_verify()["read_bytes"] == sum(FLENS)


def test_spawn_hybrid_at_32_mib(pool):
    _, parts, pads, lw, v1, rows = torrent()
    for i in range(2):
        pool.spawn_hybrid(i, 9, parts[i], len(parts[i]), pads[i], v1[i], rows[i], log2w=lw[i])
    pool.flush()
    got, deadline = [], time.monotonic() + 20.0
    while len(got) < 2 and time.monotonic() < deadline:  # no blocking call, no sleep
        got.extend(pool.try_iter_hybrid())
    assert sorted((r.index, r.conn_id, r.matched, r.sha1, r.root) for r in got) == \
        [(i, 9, 3, v1[i], rows[i]) for i in range(2)]
    assert pool.pending == 0 and pool.try_iter() == [] and pool.try_iter_merkle() == []
