"""GPU: BitTorrent v2 (BEP 52) piece verification — the SHA-256 leaf and node
kernels behind vx_merkle_device_* and vx_merkle_verify_batch.

The yardstick is hashlib.sha256 and the pure-Python BEP 52 tree below (leaves
over 16 KiB blocks, the last at its real length; zero hashes beyond the
piece; node = SHA-256(left || right); pad hashes for a layer).  Everything is
bit-exact.  Before each call the gaps between pieces and the whole leaves
buffer are 0xFF, so a read past a piece's end or an unwritten leaf row shows
up as a mismatch.
"""
import hashlib
import mmap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
ABC = b"abc"
ABC_SHA256 = "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
NOPQ = b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"
NOPQ_SHA256 = "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"


def sha256(b):
    return hashlib.sha256(b).digest()


def pad(h):
    out = bytes(32)
    for _ in range(h):
        out = sha256(out + out)
    return out


def leaf_rows(data, log2_width):
    return [sha256(data[o:o + BLOCK]) if o < len(data) else bytes(32) for o in range(0, BLOCK << log2_width, BLOCK)]


def tree_root(rows):
    while len(rows) > 1:
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
    return rows[0]


def layer_root(layer, height):
    """A layer of hashes `height` levels above the leaves, padded to the next
    power of two with pad(height), each level above with the next pad hash."""
    rows, h = list(layer), height
    while len(rows) > 1:
        if len(rows) & 1:
            rows.append(pad(h))
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
        h += 1
    return rows[0]


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Batch:
    """Pieces laid out in one 0xFF-filled buffer at 16-byte aligned offsets
    with a gap after each, and what BEP 52 says about them."""

    def __init__(self, pieces, log2_width, log2w=None, gap=48):
        self.pieces, self.log2_width = pieces, log2_width
        self.log2w = list(log2w) if log2w is not None else [log2_width] * len(pieces)
        self.offs, o = [], 0
        for p in pieces:
            self.offs.append(o)
            o += (len(p) + 15) // 16 * 16 + gap
        buf = bytearray(b"\xff" * max(o, 16))
        for p, off in zip(pieces, self.offs):
            buf[off:off + len(p)] = p
        self.buf = bytes(buf)
        self.leaves = [leaf_rows(p, log2_width) for p in pieces]
        self.roots = [tree_root(rows[:1 << w]) for rows, w in zip(self.leaves, self.log2w)]

    def run(self, dev, expected=None, per_piece=False, stream=None, leaves=None):
        import torch

        from vortex_amd import device as vdev

        n = len(self.pieces)
        data = torch.frombuffer(bytearray(self.buf), dtype=torch.uint8).to(dev)
        if leaves is None:
            leaves = torch.full(((n << self.log2_width), 32), 0xFF, dtype=torch.uint8, device=dev)
        roots = torch.full((n, 32), 0xFF, dtype=torch.uint8, device=dev)
        exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).to(dev) if expected else None
        lw = torch.tensor(self.log2w, dtype=torch.uint8, device=dev) if per_piece else None
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(dev))
        r, lv, m = vdev.merkle_ragged(data, torch.tensor(self.offs, dtype=torch.int64, device=dev),
                                      torch.tensor([len(p) for p in self.pieces], dtype=torch.int32, device=dev),
                                      self.log2_width, log2w=lw, expected=exp, leaves=leaves, roots=roots,
                                      stream=stream)
        (stream or torch.cuda.current_stream(dev)).synchronize()
        return r.cpu().numpy().tobytes(), lv.cpu().numpy().tobytes(), (m.cpu().tolist() if m is not None else None)

    def check(self, got_roots, got_leaves):
        want_leaves = b"".join(b"".join(rows) for rows in self.leaves)
        for i in range(len(self.pieces)):
            assert got_roots[32 * i:32 * i + 32] == self.roots[i], f"root of piece {i} ({len(self.pieces[i])} bytes)"
        if got_leaves != want_leaves:
            w = 1 << self.log2_width
            bad = [k for k in range(len(want_leaves) // 32) if got_leaves[32 * k:32 * k + 32] != want_leaves[32 * k:32 * k + 32]]
            raise AssertionError(f"{len(bad)} leaf rows differ, first: piece {bad[0] // w} slot {bad[0] % w}")


def piece_lengths(log2_width):
    """The issue's lengths for a tree of 2^log2_width leaf slots."""
    full = BLOCK << log2_width
    return [full, 1, BLOCK, BLOCK + 1, full // 2 + 1, full - 1]


def test_plain_sha256_ragged(built, gpu):
    """log2_width = 0: a piece's root is the SHA-256 of its bytes."""
    lens = [1, 3, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 16383, 16384]
    pieces = [random_bytes(100 + L, L) for L in lens]
    pieces[lens.index(3)] = ABC
    pieces[lens.index(56)] = NOPQ
    b = Batch(pieces, 0)
    roots, leaves, _ = b.run(gpu)
    assert roots[32 * lens.index(3):][:32].hex() == ABC_SHA256
    assert roots[32 * lens.index(56):][:32].hex() == NOPQ_SHA256
    for i, p in enumerate(pieces):
        assert roots[32 * i:32 * i + 32] == sha256(p), f"{len(p)} bytes"
    assert leaves == roots  # one leaf slot per piece: the leaf layer is the roots
    b.check(roots, leaves)


@pytest.mark.parametrize("n", [257, 512, 513, 1500])
def test_plain_sha256_many_pieces(built, gpu, n):
    """log2_width = 0 with more pieces than a node workgroup has threads: a
    tile of 512 rows is 512 pieces, two per thread."""
    lens = [(i * 37) % 301 if i % 50 else (BLOCK, BLOCK - 1, 0)[(i // 50) % 3] for i in range(n)]
    pieces = [random_bytes(5000 + i, L) for i, L in enumerate(lens)]
    b = Batch(pieces, 0)
    for per_piece in (False, True):
        roots, leaves, matched = b.run(gpu, expected=b.roots, per_piece=per_piece)
        b.check(roots, leaves)
        assert matched == [1] * n
    assert lens[100] == 0 and roots[3200:3232] == bytes(32)  # an empty piece of width 1: pad(0), the zero hash


@pytest.mark.parametrize("log2_width,n", [(1, 1), (1, 63), (1, 65), (1, 257), (4, 1), (4, 63), (4, 65), (4, 257),
                                          (7, 6), (10, 2)])
def test_trees_ragged(built, gpu, log2_width, n):
    """Roots and the whole leaf layer, zero rows included.  Width 1,024 (one
    full 16 MiB piece and a short one) takes the node kernel's multi-pass path."""
    lens = piece_lengths(log2_width)
    if log2_width == 10:
        lens = [lens[0], lens[3]]
    pieces = [random_bytes(1000 * log2_width + i, lens[i % len(lens)]) for i in range(n)]
    b = Batch(pieces, log2_width)
    roots, leaves, _ = b.run(gpu)
    b.check(roots, leaves)


@pytest.mark.parametrize("log2_width,n,length,last_len", [(1, 5, 2 * BLOCK, 1), (1, 65, BLOCK + 1, BLOCK),
                                                          (4, 5, 16 * BLOCK, BLOCK + 1), (4, 67, 8 * BLOCK + 1, 77),
                                                          (7, 3, 128 * BLOCK - 1, 64 * BLOCK + 1),
                                                          (10, 2, 1024 * BLOCK, 3 * BLOCK + 5)])
def test_trees_uniform(built, gpu, log2_width, n, length, last_len):
    """The uniform entry, with last_len < len and a stride > len."""
    import torch

    from vortex_amd import device as vdev

    stride = (length + 15) // 16 * 16 + 4096
    pieces = [random_bytes(7000 + 10 * log2_width + i, length if i < n - 1 else last_len) for i in range(n)]
    buf = bytearray(b"\xff" * ((n - 1) * stride + (last_len + 15) // 16 * 16))
    for i, p in enumerate(pieces):
        buf[i * stride:i * stride + len(p)] = p
    data = torch.frombuffer(buf, dtype=torch.uint8).to(gpu)
    leaves = torch.full((n << log2_width, 32), 0xFF, dtype=torch.uint8, device=gpu)
    want_rows = [leaf_rows(p, log2_width) for p in pieces]
    want_roots = [tree_root(rows) for rows in want_rows]
    expected = torch.frombuffer(bytearray(b"".join(want_roots)), dtype=torch.uint8).to(gpu)
    roots, leaves, matched = vdev.merkle_uniform(data, n, length, log2_width, stride=stride, last_len=last_len,
                                                 expected=expected, leaves=leaves)
    torch.cuda.synchronize()
    assert roots.cpu().numpy().tobytes() == b"".join(want_roots)
    assert leaves.cpu().numpy().tobytes() == b"".join(b"".join(rows) for rows in want_rows)
    assert matched.cpu().tolist() == [1] * n


def test_per_piece_log2w(built, gpu):
    """Single-piece files inside a log2_width = 4 batch: each root comes from
    the level of the piece's own width, the leaf rows stay 16 per piece."""
    lens_w = [(1, 0), (BLOCK, 0), (BLOCK + 1, 1), (2 * BLOCK, 1), (2 * BLOCK + 1, 2), (3 * BLOCK + 5, 2), (100, 1),
              (BLOCK - 1, 2), (16 * BLOCK, 4), (9 * BLOCK + 9, 4), (4 * BLOCK, 2)]
    pieces = [random_bytes(300 + i, L) for i, (L, _) in enumerate(lens_w)]
    b = Batch(pieces, 4, log2w=[w for _, w in lens_w])
    roots, leaves, _ = b.run(gpu, per_piece=True)
    b.check(roots, leaves)
    assert roots[:32] == sha256(pieces[0])  # width 1: the root is the leaf
    assert roots[32 * 2:32 * 3] == sha256(sha256(pieces[2][:BLOCK]) + sha256(pieces[2][BLOCK:]))


@pytest.mark.parametrize("log2_width", [0, 4, 10])
def test_empty_piece_beside_full_ones(built, gpu, log2_width):
    full = BLOCK << log2_width
    pieces = [random_bytes(41, full), b"", random_bytes(42, full)]
    b = Batch(pieces, log2_width)
    assert b.roots[1] == pad(log2_width)
    roots, leaves, _ = b.run(gpu)
    b.check(roots, leaves)
    assert roots[32:64] == pad(log2_width)


def test_verdict_one_flipped_byte(built, gpu):
    log2_width, n, bad_piece, bad_leaf = 4, 9, 5, 11
    full = BLOCK << log2_width
    clean = [random_bytes(500 + i, full if i != 7 else full - 3) for i in range(n)]
    want = Batch(clean, log2_width)
    dirty = list(clean)
    flipped = bytearray(clean[bad_piece])
    flipped[bad_leaf * BLOCK + 1234] ^= 0x10
    dirty[bad_piece] = bytes(flipped)
    roots, leaves, matched = Batch(dirty, log2_width).run(gpu, expected=want.roots)
    assert matched == [int(i != bad_piece) for i in range(n)]
    clean_leaves = b"".join(b"".join(rows) for rows in want.leaves)
    differ = [k for k in range(n << log2_width) if leaves[32 * k:32 * k + 32] != clean_leaves[32 * k:32 * k + 32]]
    assert differ == [(bad_piece << log2_width) + bad_leaf]
    assert [roots[32 * i:32 * i + 32] == want.roots[i] for i in range(n)] == [i != bad_piece for i in range(n)]
    # and with the clean data every piece matches
    _, _, matched = want.run(gpu, expected=want.roots)
    assert matched == [1] * n


def test_streams_and_reused_leaves(built, gpu):
    """A non-default stream, and two calls back to back into one leaves
    buffer: the second call's rows replace all of the first's."""
    import torch

    log2_width, n = 4, 6
    a = Batch([random_bytes(600 + i, BLOCK << log2_width) for i in range(n)], log2_width)
    b = Batch([random_bytes(700 + i, L) for i, L in enumerate(piece_lengths(log2_width))], log2_width)
    stream = torch.cuda.Stream(device=gpu)
    leaves = torch.full((n << log2_width, 32), 0xFF, dtype=torch.uint8, device=gpu)
    roots_a, leaves_a, _ = a.run(gpu, stream=stream, leaves=leaves)
    a.check(roots_a, leaves_a)
    roots_b, leaves_b, _ = b.run(gpu, stream=stream, leaves=leaves)  # stale rows of `a` where b has zero rows
    b.check(roots_b, leaves_b)


@pytest.mark.parametrize("height", [0, 4])
def test_merkle_root_of_a_layer(built, gpu, height):
    import torch

    from vortex_amd import device as vdev

    for n in (1, 2, 3, 5, 64, 65, 1000):
        layer = [sha256(b"%d/%d" % (k, n)) for k in range(n)]
        raw = b"".join(layer)
        d_layer = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gpu).reshape(n, 32)
        root = vdev.merkle_root(d_layer, height)
        torch.cuda.synchronize()
        assert root.cpu().numpy().tobytes() == layer_root(layer, height), n
        assert d_layer.cpu().numpy().tobytes() == raw  # the layer is not modified
    # piece layers -> pieces root: the roots of a file's pieces reduce to the file's root
    pieces = [random_bytes(900 + i, L) for i, L in enumerate([4 * BLOCK] * 4 + [BLOCK + 9])]
    b = Batch(pieces, 2)
    roots, _, _ = b.run(gpu)
    d_roots = torch.frombuffer(bytearray(roots), dtype=torch.uint8).to(gpu)
    whole = tree_root(leaf_rows(b"".join(pieces), 5))  # 17 blocks -> 32 leaf slots
    got = vdev.merkle_root(d_roots, 2)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == whole == layer_root(b.roots, 2)


def test_ragged_layout_check_refuses_without_launching(built, gpu):
    import torch

    from vortex_amd import device as vdev

    data = torch.zeros(4 * BLOCK + 64, dtype=torch.uint8, device=gpu)
    leaves = torch.full((2 << 2, 32), 0xFF, dtype=torch.uint8, device=gpu)

    def call(offs, lens, log2w=None):
        lw = torch.tensor(log2w, dtype=torch.uint8, device=gpu) if log2w is not None else None
        return vdev.merkle_ragged(data, torch.tensor(offs, dtype=torch.int64, device=gpu),
                                  torch.tensor(lens, dtype=torch.int32, device=gpu), 2, log2w=lw, leaves=leaves)

    with pytest.raises(ValueError, match="multiple of 16"):
        call([0, 2 * BLOCK + 8], [BLOCK, BLOCK])
    with pytest.raises(ValueError, match="past the data tensor"):
        call([0, 2 * BLOCK], [BLOCK, 2 * BLOCK + 65])
    with pytest.raises(ValueError, match="log2w 3 > log2_width 2"):
        call([0, 2 * BLOCK], [BLOCK, BLOCK], log2w=[0, 3])
    with pytest.raises(ValueError, match="longer than its tree"):
        call([0, BLOCK], [BLOCK, BLOCK + 1], log2w=[0, 0])
    torch.cuda.synchronize()
    assert bool((leaves == 0xFF).all())  # nothing ran
    roots, _, _ = call([0, 2 * BLOCK], [BLOCK, 2 * BLOCK + 64], log2w=[0, 2])  # the same shapes, legal
    torch.cuda.synchronize()
    assert roots.cpu().numpy().tobytes() == tree_root(leaf_rows(bytes(BLOCK), 0)) + \
        tree_root(leaf_rows(bytes(2 * BLOCK + 64), 2))


def test_hash_pool_verify_merkle(built, gpu):
    """vx_merkle_verify_batch: 37 pieces of mixed lengths at piece_length
    256 KiB, one corrupted, from plain and from registered memory; the stats
    add up, and the pool's SHA-1 batch gives the same answers before and after."""
    from vortex_amd.hash_pool import HashPool

    piece_length, n, bad = 256 * 1024, 37, 23
    lens = [piece_length] * n
    for i, L in ((3, 1), (8, BLOCK), (12, BLOCK + 1), (17, piece_length // 2 + 1), (29, piece_length - 1), (31, 0),
                 (36, 5 * BLOCK + 5)):
        lens[i] = L
    pieces = [random_bytes(2000 + i, L) for i, L in enumerate(lens)]
    roots = [tree_root(leaf_rows(p, 4)) for p in pieces]
    sent = list(pieces)
    flipped = bytearray(pieces[bad])
    flipped[200000] ^= 1
    sent[bad] = bytes(flipped)
    sent_roots = list(roots)
    sent_roots[bad] = tree_root(leaf_rows(sent[bad], 4))
    sha1_pieces = [random_bytes(3000 + i, L) for i, L in enumerate([piece_length, 70000, 1, 0, 12345])]
    sha1_want = [hashlib.sha1(p).digest() for p in sha1_pieces]

    # slot_bytes of 9 pieces: the batch takes several rounds over the two slots
    with HashPool(piece_length, slots=2, slot_bytes=9 * piece_length) as pool:
        def sha1_ok():
            matched, digests = pool.verify_batch(sha1_pieces, sha1_want[:-1] + [bytes(20)])
            assert digests == sha1_want and matched == [True] * 4 + [False]

        sha1_ok()
        st0 = pool.stats()
        matched, got = pool.verify_merkle([bytearray(p) for p in sent], roots, piece_length)
        assert matched == [i != bad for i in range(n)]
        assert got == sent_roots
        st1 = pool.stats()
        assert st1["pieces_completed"] - st0["pieces_completed"] == n
        assert st1["pieces_mismatched"] - st0["pieces_mismatched"] == 1
        assert st1["bytes_completed"] - st0["bytes_completed"] == sum(lens)
        assert st1["staged_bytes"] - st0["staged_bytes"] == sum(lens)
        assert st1["batches"] - st0["batches"] == 5  # 9 pieces of room per round, 37 pieces
        sha1_ok()

        # the same pieces from a registered buffer: copied from where they lie
        pinned = mmap.mmap(-1, n * piece_length)
        pool.register_buffer(pinned)
        views = []
        for i, p in enumerate(sent):
            view = memoryview(pinned)[i * piece_length:i * piece_length + len(p)]
            view[:] = p
            views.append(view)
        st1 = pool.stats()
        matched, got = pool.verify_merkle(views, roots, piece_length)
        assert matched == [i != bad for i in range(n)] and got == sent_roots
        st2 = pool.stats()
        assert st2["pieces_completed"] - st1["pieces_completed"] == n
        assert st2["pieces_mismatched"] - st1["pieces_mismatched"] == 1
        assert st2["bytes_completed"] - st1["bytes_completed"] == sum(lens)
        assert st2["staged_bytes"] == st1["staged_bytes"]  # nothing went through the stage
        sha1_ok()
        del views, view
        pool.unregister_buffer(pinned)

        # a single-piece file keeps its own width; a piece longer than its tree is refused
        short = random_bytes(77, 3 * BLOCK + 5)
        matched, got = pool.verify_merkle([short], [tree_root(leaf_rows(short, 2))], piece_length, log2w=[2])
        assert matched == [True] and got == [tree_root(leaf_rows(short, 2))]
        from vortex_amd._lib import VX_EINVAL, VX_ERANGE, VxError

        for args, code in ((([short], [bytes(32)], piece_length, [1]), VX_EINVAL),
                           (([short], [bytes(32)], piece_length, [5]), VX_EINVAL),
                           (([short], [bytes(32)], piece_length * 2), VX_ERANGE),
                           (([short], [bytes(32)], piece_length + BLOCK), VX_EINVAL)):
            with pytest.raises(VxError) as e:
                pool.verify_merkle(*args)
            assert e.value.code == code
        assert pool.verify_merkle([], [], piece_length) == ([], [])
        sha1_ok()
