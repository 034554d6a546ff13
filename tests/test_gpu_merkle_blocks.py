"""GPU: the block checks (vx_merkle_device_block_check, vx_merkle_check_blocks)
against hashlib, bit-exact: which 16 KiB blocks of a v2 piece differ from their
expected leaf rows, as a bitmap, and the leaf rows themselves.  Every output
tensor the tests own is filled with 0xFF and has one spare word or row that
must stay 0xFF; the arena between the pieces is random garbage, so a read past
a piece's end shows as a wrong leaf."""
import ctypes
import hashlib
import mmap
import random

import pytest

from test_gpu_merkle_async import collect, model_root
from test_merkle_blocks_cpu import _leaves, _reduce

pytestmark = pytest.mark.gpu
BLOCK = 16384
KiB = 1024

# (log2_width, n): 64 and 2 pieces per wave, one wave per piece, multi-wave pieces, more than one
# workgroup per piece.  n << log2_width is a multiple of neither 64 nor 256 where the width allows
# it (67, 134, 608; from width 6 on every count is a multiple of 64: 1216 = 4.75 x 256, 2432 =
# 9.5 x 256; from width 8 on of 256 too), and of both in the case (1, 128).
CASES = [(0, 67), (1, 67), (5, 19), (6, 19), (7, 19), (8, 17), (9, 17), (1, 128), (7, 3)]


def sha256(b):
    return hashlib.sha256(b).digest()


def _lengths(lw, n, rng):
    """Piece lengths of one batch: the edges the issue names, cut to the width."""
    cap = BLOCK << lw
    want = [0, 1, 16383, 16384, 16385, cap]
    # last blocks of len % 128 in {0, 1, 55, 56, 63, 64, 119, 120, 127}: one, two and three tail compressions
    want += [min(cap - BLOCK, 2 * BLOCK) + 128 * 3 + r for r in (0, 1, 55, 56, 63, 64, 119, 120, 127)]
    if lw >= 7:
        want.append(65 * BLOCK + 55)  # blocks 63 and 64: the edge of a bitmap word
    want = [x for x in want if x <= cap]
    while len(want) < n:
        want.append(rng.randrange(0, min(cap, 3 * BLOCK) + 1))
    return want[:n] if n >= len(want) else [cap, 16385 if cap > BLOCK else 16383, 0][:n]


class Batch:
    """n pieces in one arena of garbage at 16-byte aligned offsets, at least 16 bytes apart."""

    def __init__(self, lw, n, seed):
        rng = random.Random(seed)
        self.lw, self.W, self.n = lw, 1 << lw, n
        self.lens = _lengths(lw, n, rng)
        assert len(self.lens) == n
        self.offs, at = [], 0
        for L in self.lens:
            self.offs.append(at)
            at += (L + 15) // 16 * 16 + 16
        self.arena = bytearray(rng.randbytes(at))
        self.pieces = [bytes(self.arena[o:o + L]) for o, L in zip(self.offs, self.lens)]
        self.leaves = [_leaves(p, self.W) for p in self.pieces]  # hashlib, computed once
        self.wpp = max(1, self.W // 64)

    def tensors(self, dev, arena=None):
        import torch

        return (torch.frombuffer(bytearray(arena if arena is not None else self.arena), dtype=torch.uint8).to(dev),
                torch.tensor(self.offs, dtype=torch.int64, device=dev),
                torch.tensor(self.lens, dtype=torch.int32, device=dev))

    def words(self, bad_lists):
        out = [0] * (self.n * self.wpp)
        for i, bl in enumerate(bad_lists):
            for b in bl:
                out[i * self.wpp + (b >> 6)] |= 1 << (b & 63)
        return out


_batches = {}


def batch(lw, n):
    if (lw, n) not in _batches:
        _batches[(lw, n)] = Batch(lw, n, 0xB10C5 + 1000 * lw + n)
    return _batches[(lw, n)]


def _rows_tensor(rows, dev):
    import torch

    return torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev).view(-1, 32)


def _run(b, dev, arena, exp_rows, want_leaves=True):
    """One call with 0xFF-filled outputs of one spare word / row; returns (words, leaf bytes)."""
    import torch

    from vortex_amd import device as vdev

    data, offs, lens = b.tensors(dev, arena)
    nw, rows = b.n * b.wpp, b.n * b.W
    bad = torch.full((nw + 1,), -1, dtype=torch.int64, device=dev)
    leaves = torch.full((rows + 1, 32), 0xFF, dtype=torch.uint8, device=dev) if want_leaves else None
    exp = _rows_tensor(exp_rows, dev)
    got_bad, got_leaves = vdev.merkle_block_check(data, offs, lens, b.lw, expected_leaves=exp, leaves=leaves, bad=bad)
    torch.cuda.synchronize()
    assert got_bad is bad and got_leaves is leaves
    assert exp.cpu().numpy().tobytes() == b"".join(exp_rows)  # inputs untouched
    words = bad.cpu().numpy().view("uint64").tolist()
    assert words[nw] == 0xFFFFFFFFFFFFFFFF, "the word past the bitmap was written"
    raw = None
    if want_leaves:
        raw = leaves.cpu().numpy().tobytes()
        assert raw[32 * rows:] == b"\xFF" * 32, "the row past the leaves was written"
        raw = raw[:32 * rows]
    return words[:nw], raw


def _garbage_past_end(b, rng):
    """The good leaf rows, with garbage in every slot at or past its piece's end."""
    rows = []
    for i in range(b.n):
        used = (b.lens[i] + BLOCK - 1) // BLOCK
        rows += b.leaves[i][:used] + [rng.randbytes(32) for _ in range(b.W - used)]
    return rows


@pytest.mark.parametrize("lw,n", CASES)
def test_clean_batch_writes_every_word_as_zero(built, gpu, lw, n):
    """No damage: every word comes back 0 out of a 0xFF-filled bitmap, garbage
    expected rows beyond the pieces' ends do not flag, and the leaves are
    hashlib's and merkle_ragged's, byte for byte."""
    import torch

    from vortex_amd import device as vdev

    b = batch(lw, n)
    words, raw = _run(b, gpu, None, _garbage_past_end(b, random.Random(lw * 100 + n)))
    assert words == [0] * (n * b.wpp)
    assert raw == b"".join(b"".join(lv) for lv in b.leaves)
    data, offs, lens = b.tensors(gpu)
    _, ragged, _ = vdev.merkle_ragged(data, offs, lens, lw)
    torch.cuda.synchronize()
    assert ragged.cpu().numpy().tobytes() == raw


@pytest.mark.parametrize("lw,n", CASES)
def test_damage_patterns(built, gpu, lw, n):
    """Every block of one piece; the first block only (its first byte); the last,
    short block only (its last byte); blocks 63 and 64; expected rows off in
    their first or their last word only; garbage rows and garbage bytes past
    the pieces' ends."""
    b = batch(lw, n)
    rng = random.Random(0xDA7A + lw * 100 + n)
    arena = bytearray(b.arena)
    exp = [list(lv) for lv in b.leaves]
    want = [set() for _ in range(n)]
    nblocks = [(L + BLOCK - 1) // BLOCK for L in b.lens]

    def flip(i, off):
        arena[b.offs[i] + off] ^= 0x10
        want[i].add(off // BLOCK)

    def first(pred, taken):
        for i in range(n):
            if i not in taken and pred(i):
                taken.add(i)
                return i
        return None

    taken = set()
    full = first(lambda i: b.lens[i] == BLOCK << lw, taken)
    for k in range(b.W):  # every block, at a different byte each
        flip(full, k * BLOCK + (k * 977) % BLOCK)
    i = first(lambda i: nblocks[i] >= 2, taken) if lw else first(lambda i: b.lens[i] == 16383, taken)
    flip(i, 0)  # the first block only, by its first byte
    i = first(lambda i: b.lens[i] % BLOCK and (nblocks[i] >= 2 or not lw), taken)
    if i is not None:
        flip(i, b.lens[i] - 1)  # the last, short block only, by its last byte
    i = first(lambda i: b.lens[i] and b.lens[i] % BLOCK == 0, taken)
    if i is not None:
        flip(i, BLOCK - 1)  # the last byte of a full block
    i = first(lambda i: nblocks[i] >= 65, taken)
    if i is not None:  # the word edge
        flip(i, 63 * BLOCK + 5)
        flip(i, 64 * BLOCK + 7)
    i = first(lambda i: nblocks[i] >= 1, taken)
    if i is not None:
        exp[i][0] = bytes([exp[i][0][0] ^ 0x80]) + exp[i][0][1:]  # off in its first word only
        want[i].add(0)
    i = first(lambda i: nblocks[i] >= 1, taken)
    if i is not None:
        k = nblocks[i] - 1
        exp[i][k] = exp[i][k][:31] + bytes([exp[i][k][31] ^ 1])  # off in its last word only
        want[i].add(k)
    # the small batch (7, 3) has three pieces to damage; every other one takes all the patterns
    assert len(taken) == (2 if n == 3 else 7 if lw >= 7 else 6)
    for i in range(n):  # garbage rows beyond every piece's end
        for k in range(nblocks[i], b.W):
            exp[i][k] = rng.randbytes(32)
    exp_rows = [r for rows in exp for r in rows]
    # the model, from hashlib alone, and what was built into it
    damaged = [bytes(arena[o:o + L]) for o, L in zip(b.offs, b.lens)]
    model = [[k for k in range(nblocks[i]) if sha256(damaged[i][k * BLOCK:(k + 1) * BLOCK]) != exp[i][k]]
             for i in range(n)]
    assert model == [sorted(w) for w in want]
    assert model[full] == list(range(b.W)) and sum(map(len, model)) >= b.W + 1

    words, raw = _run(b, gpu, arena, exp_rows)
    assert words == b.words(model)
    assert raw == b"".join(b"".join(_leaves(d, b.W)) for d in damaged)
    # the bitmap alone is the same bitmap
    words2, none = _run(b, gpu, arena, exp_rows, want_leaves=False)
    assert none is None and words2 == words
    # every block of every piece against rows of garbage: all the blocks there are, and no more
    words3, _ = _run(b, gpu, None, [rng.randbytes(32) for _ in range(n * b.W)], want_leaves=False)
    assert words3 == b.words([range(k) for k in nblocks])


def test_every_word_of_a_leaf_row_decides(built, gpu):
    """64 blocks of one piece, 32 to 95 of its 128, so both of its bitmap words:
    the stored leaf row of block k is one bit off, in word k % 8 (the bit moves
    through the word with k).  The bitmap names exactly those blocks; a compare
    that skipped one of the eight words would miss eight of them."""
    lw, n = 7, 19
    b = batch(lw, n)
    victim = b.lens.index(BLOCK << lw)
    blocks = list(range(32, 96))
    exp = _garbage_past_end(b, random.Random(0x0B17))
    for k in blocks:
        row = bytearray(exp[victim * b.W + k])
        assert bytes(row) == b.leaves[victim][k]
        bit = (5 * k + 3) % 32
        row[4 * (k % 8) + bit // 8] ^= 1 << (bit % 8)
        exp[victim * b.W + k] = bytes(row)
    assert {k % 8 for k in blocks} == set(range(8)) and len({(5 * k + 3) % 32 for k in blocks}) == 32
    want = [blocks if i == victim else [] for i in range(n)]
    words, raw = _run(b, gpu, None, exp)
    assert words == b.words(want)
    assert words[victim * b.wpp:(victim + 1) * b.wpp] == [0xFFFFFFFF00000000, 0x00000000FFFFFFFF]
    assert raw == b"".join(b"".join(lv) for lv in b.leaves)  # the leaves written are the data's, not the stored rows


def test_leaves_only_form(built, gpu):
    import torch

    from vortex_amd import device as vdev

    b = batch(5, 19)
    data, offs, lens = b.tensors(gpu)
    leaves = torch.full((b.n * b.W + 1, 32), 0xFF, dtype=torch.uint8, device=gpu)
    bad, got = vdev.merkle_block_check(data, offs, lens, b.lw, leaves=leaves)
    torch.cuda.synchronize()
    assert bad is None and got is leaves
    raw = leaves.cpu().numpy().tobytes()
    assert raw == b"".join(b"".join(lv) for lv in b.leaves) + b"\xFF" * 32
    bad, got = vdev.merkle_block_check(data, offs, lens, b.lw)  # allocated here
    torch.cuda.synchronize()
    assert bad is None and got.cpu().numpy().tobytes() == raw[:-32]


def test_empty_batch_and_refusals(built, gpu):
    import torch

    from vortex_amd import _lib
    from vortex_amd import device as vdev

    b = batch(1, 67)
    data, offs, lens = b.tensors(gpu)
    exp = _rows_tensor([r for lv in b.leaves for r in lv], gpu)
    bad, leaves = vdev.merkle_block_check(data, offs[:0], lens[:0], 3, expected_leaves=exp[:0], want_leaves=True)
    assert bad.numel() == 0 and leaves.numel() == 0
    with pytest.raises(ValueError, match="neither"):
        vdev.merkle_block_check(data, offs, lens, 1, want_leaves=False)
    with pytest.raises(ValueError, match="expected_leaves must hold"):
        vdev.merkle_block_check(data, offs, lens, 1, expected_leaves=exp[:-1])
    with pytest.raises(ValueError, match="bad needs"):
        vdev.merkle_block_check(data, offs, lens, 1, bad=torch.zeros(67, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError, match="bad must hold"):
        vdev.merkle_block_check(data, offs, lens, 1, expected_leaves=exp,
                                bad=torch.zeros(66, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError, match="longer than its tree"):
        vdev.merkle_block_check(data, offs, lens, 0, expected_leaves=exp)
    with pytest.raises(ValueError, match="multiple of 16"):
        vdev.merkle_block_check(data, offs + 8, lens, 1, expected_leaves=exp)
    with pytest.raises(ValueError, match="past the data tensor"):
        vdev.merkle_block_check(data[:-64], offs, lens, 1, expected_leaves=exp)
    # the C entry itself, on real device pointers
    fn, E = _lib.lib().vx_merkle_device_block_check, _lib.VX_EINVAL
    words = torch.zeros(68, dtype=torch.int64, device=gpu)
    out = torch.zeros((134, 32), dtype=torch.uint8, device=gpu)
    args = [data.data_ptr(), offs.data_ptr(), lens.data_ptr(), 67, 1, exp.data_ptr(), words.data_ptr(), out.data_ptr(),
            None]
    for k, v in ((0, None), (1, None), (2, None), (4, 18), (5, None), (6, None), (0, data.data_ptr() + 8),
                 (5, exp.data_ptr() + 8), (6, words.data_ptr() + 4), (7, out.data_ptr() + 8)):
        a = list(args)
        a[k] = v
        assert fn(*a) == E, k
    a = list(args)
    a[5] = a[6] = a[7] = None
    assert fn(*a) == E
    torch.cuda.synchronize()
    assert not words.any() and not out.any()  # a refused call launches nothing


# ---- the context call ----------------------------------------------------------------------

PLEN, LW = 128 * KiB, 3


def _file_pieces(seed, n=9):
    """n pieces of a file at 128 KiB pieces: full ones, the last 2 blocks and 9 bytes."""
    body = random.Random(seed).randbytes((n - 1) * PLEN + 2 * BLOCK + 9)
    return [body[o:o + PLEN] for o in range(0, len(body), PLEN)]


def _damage(pieces):
    """(damaged pieces, the bad blocks of each)."""
    hits = {0: [0], 2: [0, 5], 3: [7], 5: list(range(8)), len(pieces) - 1: [2]}
    out = []
    for i, p in enumerate(pieces):
        p = bytearray(p)
        for k in hits.get(i, []):
            p[min(k * BLOCK + 100 * k, len(p) - 1)] ^= 0x04
        out.append(bytes(p))
    return out, [hits.get(i, []) for i in range(len(pieces))]


@pytest.mark.parametrize("registered", [False, True])
def test_check_blocks_in_rounds(built, gpu, registered):
    """9 pieces through a context whose slot_bytes holds two of them: five
    rounds, over plain and over registered memory; the bitmap, bad_counts_out
    and leaves_out of the C call, and stats() untouched."""
    from vortex_amd import merkle
    from vortex_amd.hash_pool import HashPool

    pieces = _file_pieces(0xC0FFEE)
    n = len(pieces)
    good_leaves = [b"".join(_leaves(p, 8)) for p in pieces]
    damaged, hits = _damage(pieces)
    with HashPool(PLEN, slots=2, slot_bytes=2 * PLEN) as pool:
        bufs = damaged
        if registered:
            reg = mmap.mmap(-1, n * PLEN)
            pool.register_buffer(reg)
            for i, p in enumerate(damaged):
                reg[i * PLEN:i * PLEN + len(p)] = p
            bufs = [memoryview(reg)[i * PLEN:i * PLEN + len(p)] for i, p in enumerate(damaged)]
        before = pool.stats()
        bad, leaves = pool.check_blocks(bufs, PLEN, good_leaves, want_leaves=True)
        assert bad == hits == [merkle.bad_blocks(d, g) for d, g in zip(damaged, good_leaves)]
        assert leaves == [b"".join(_leaves(d, 8)) for d in damaged]
        assert pool.check_blocks(bufs, PLEN, good_leaves) == (hits, None)
        assert pool.check_blocks(bufs, PLEN, want_leaves=True) == (None, leaves)
        assert pool.check_blocks(bufs, PLEN, leaves) == ([[] for _ in range(n)], None)
        assert pool.check_blocks([], PLEN, []) == ([], None)
        # the C call's own outputs, 0xFF-filled first
        from vortex_amd.hash_pool import _ptr_arrays

        ptrs, lens, keep = _ptr_arrays(bufs)
        exp = ctypes.create_string_buffer(b"".join(good_leaves), 256 * n)
        words = (ctypes.c_uint64 * (n + 1))(*[0xFFFFFFFFFFFFFFFF] * (n + 1))
        counts = (ctypes.c_uint32 * (n + 1))(*[0xFFFFFFFF] * (n + 1))
        fn = pool.lib.vx_merkle_check_blocks
        assert fn(pool._h, ptrs, lens, n, PLEN, exp, words, counts, None) == 0
        assert list(words) == [sum(1 << k for k in h) for h in hits] + [0xFFFFFFFFFFFFFFFF]
        assert list(counts) == [len(h) for h in hits] + [0xFFFFFFFF]
        assert pool.stats() == before and pool.pending == 0
        if registered:
            del bufs, ptrs, keep
            pool.unregister_buffer(reg)


def test_check_blocks_wide_pieces_and_refusals(built, gpu):
    """2 MiB pieces (two bitmap words each) and what the call refuses."""
    from vortex_amd import _lib
    from vortex_amd._lib import VxError
    from vortex_amd.hash_pool import HashPool, _ptr_arrays

    plen = 128 * BLOCK
    rng = random.Random(0x2B175)
    pieces = [bytearray(rng.randbytes(plen)), bytearray(rng.randbytes(65 * BLOCK + 1)), bytearray()]
    good = [b"".join(_leaves(bytes(p), 128)) for p in pieces]
    for off in (63 * BLOCK, 64 * BLOCK + 1, 127 * BLOCK + BLOCK - 1):
        pieces[0][off] ^= 1
    pieces[1][64 * BLOCK] ^= 1
    with HashPool(plen, slots=2, slot_bytes=plen) as pool:
        before = pool.stats()
        bad, _ = pool.check_blocks(pieces, plen, good)
        assert bad == [[63, 64, 127], [64], []]
        ptrs, lens, keep = _ptr_arrays(pieces)
        words = (ctypes.c_uint64 * 6)()
        out = ctypes.create_string_buffer(3 * 128 * 32)
        exp = ctypes.create_string_buffer(b"".join(good), 3 * 128 * 32)
        fn, h = pool.lib.vx_merkle_check_blocks, pool._h
        E, R = _lib.VX_EINVAL, _lib.VX_ERANGE
        assert fn(h, ptrs, lens, 3, plen, exp, None, None, out) == E      # expected without a bitmap
        assert fn(h, ptrs, lens, 3, plen, None, words, None, out) == E    # a bitmap without expected
        assert fn(h, ptrs, lens, 3, plen, None, None, None, None) == E    # nothing asked for
        counts = (ctypes.c_uint32 * 3)()
        assert fn(h, ptrs, lens, 3, plen, None, None, counts, out) == E   # counts without expected
        assert fn(h, None, lens, 3, plen, exp, words, None, None) == E
        assert fn(h, ptrs, None, 3, plen, exp, words, None, None) == E
        assert fn(h, ptrs, lens, 3, plen + 16384, exp, words, None, None) == E   # not a power of two
        assert fn(h, ptrs, lens, 3, 8192, exp, words, None, None) == E
        assert fn(h, ptrs, lens, 3, 2 * plen, exp, words, None, None) == R       # > max_piece_len
        assert fn(h, ptrs, lens, 3, plen // 2, exp, words, None, None) == E      # lens[0] > piece_length
        nul = (ctypes.c_void_p * 3)(ptrs[0], None, ptrs[2])
        assert fn(h, nul, lens, 3, plen, exp, words, None, None) == E            # NULL for a non-empty piece
        nul = (ctypes.c_void_p * 3)(ptrs[0], ptrs[1], None)
        assert fn(h, nul, lens, 3, plen, exp, words, None, None) == 0            # ... but not for an empty one
        assert list(words) == [1 << 63, 1 | 1 << 63, 0, 1, 0, 0]
        assert fn(h, None, None, 0, plen, None, None, None, None) == 0           # n == 0
        assert not any(out.raw) and pool.stats() == before
        with pytest.raises(VxError):
            pool.check_blocks(pieces, 4 * plen, [g * 4 for g in good])
        with pytest.raises(ValueError):
            pool.check_blocks(pieces, plen, good[:2])
        with pytest.raises(ValueError):
            pool.check_blocks(pieces, plen)


def test_check_blocks_while_pieces_are_pending(built, gpu):
    """A block check in the middle of a download: 8 spawn_merkle pieces
    submitted and not flushed, then flushed; the answers are right both times
    and the 8 completions arrive afterwards, every one of them."""
    from vortex_amd.hash_pool import HashPool

    pieces = _file_pieces(0xBEEF, n=4)
    good_leaves = [b"".join(_leaves(p, 8)) for p in pieces]
    damaged, hits = _damage(pieces)
    rng = random.Random(0xD0)
    bodies = [rng.randbytes(PLEN if i != 7 else 3 * BLOCK + 1) for i in range(8)]
    roots = [model_root(x, LW) for x in bodies]
    with HashPool(PLEN, slots=2, batch_pieces=16) as pool:
        for i, x in enumerate(bodies):
            pool.spawn_merkle(i, 1, x, len(x), roots[i] if i != 3 else bytes(32))
        assert pool.pending == 8
        before = pool.stats()
        assert pool.check_blocks(damaged, PLEN, good_leaves) == (hits, None)
        assert pool.pending == 8 and pool.stats() == before
        pool.flush()
        bad, leaves = pool.check_blocks(damaged, PLEN, good_leaves, want_leaves=True)
        assert bad == hits and leaves == [b"".join(_leaves(d, 8)) for d in damaged]
        got = collect(pool, 8)
        assert sorted((r.index, r.hash_matched, r.digest) for r in got) == [(i, i != 3, roots[i]) for i in range(8)]
        assert pool.pending == 0 and pool.try_iter() == []


def test_seeder_to_downloader(built, gpu):
    """The loop closed: a seeder's leaves out of check_blocks, block_proof for
    every piece accepted against the file's `pieces root`, an altered leaf
    rejected, and the proven leaves finding exactly the corrupted blocks."""
    from vortex_amd import merkle
    from vortex_amd.hash_pool import HashPool

    pieces = _file_pieces(0x5EED, n=5)
    m = len(pieces)
    with HashPool(PLEN) as pool:
        _, leaves = pool.check_blocks(pieces, PLEN, want_leaves=True)                     # the seeder
        assert leaves == [b"".join(_leaves(p, 8)) for p in pieces]
        layer = [_reduce([lv[32 * k:32 * k + 32] for k in range(8)], 0) for lv in leaves]
        trees, roots = pool.build_piece_trees([b"".join(layer)], PLEN)
        root = _reduce(layer, LW)
        assert roots == [root]
        proofs = [merkle.block_proof(leaves[i], trees[0], m, LW, i, 0, 8) for i in range(m)]
        rows = len(proofs[0]) // 32
        assert rows == 8 + 3
        wire = b"".join(proofs)
        table = [(i, i * rows, 0, 8, 3) for i in range(m)]                                # the downloader
        assert pool.verify_hash_proofs(wire, table, [root]) == [True] * m
        forged = bytearray(wire)
        forged[rows * 32 * 2 + 32 * 5 + 9] ^= 1  # leaf 5 of piece 2
        assert pool.verify_hash_proofs(bytes(forged), table, [root]) == [True, True, False, True, True]
        proven = [p[:256] for p in proofs]
        assert proven == leaves
        got = [bytearray(p) for p in pieces]
        got[2][0] ^= 1
        got[2][5 * BLOCK + 4000] ^= 0x80
        got[4][len(got[4]) - 1] ^= 1
        bad, _ = pool.check_blocks(got, PLEN, proven)
        assert bad == [[], [], [0, 5], [], [2]]
