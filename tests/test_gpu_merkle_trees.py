"""GPU: the layer trees — merkle_tree_kernel behind vx_merkle_device_trees
(device.merkle_trees) and vx_merkle_build_trees (HashPool.build_piece_trees),
byte for byte against merkle.build_tree (hashlib), and proofs looked up from a
device-built tree through the existing proof verifier.

The references are computed once per module: about 0.53 M rows, one second of
hashlib per height.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one, two and three passes, and every edge of a tile
COUNTS = [1, 2, 3, 5, 511, 512, 513, 1023, 1024, 1025, 262144, 262145]
HEIGHTS = [0, 4]
PIECE_LENGTH = {0: 16384, 4: 16384 << 4}  # build_piece_trees takes the height as a piece length


def _rows(seed, n):
    return np.random.default_rng(seed).integers(0, 256, 32 * n, dtype=np.uint8).tobytes()


def _split(blob, counts):
    out, at = [], 0
    for c in counts:
        out.append(blob[32 * at:32 * (at + c)])
        at += c
    return out


@pytest.fixture(scope="module")
def edges():
    """(layers, {height: [tree per layer]}) of COUNTS."""
    from vortex_amd import merkle

    layers = _split(_rows(0x7EE, sum(COUNTS)), COUNTS)
    return layers, {h: [merkle.build_tree(x, h) for x in layers] for h in HEIGHTS}


@pytest.fixture(scope="module")
def many():
    """2,000 layers of random counts in 1..1,100: the same pair."""
    from vortex_amd import merkle

    rng = random.Random(0x2000)
    counts = [rng.randint(1, 1100) for _ in range(2000)]
    counts[:4] = [1, 1100, 512, 513]
    layers = _split(_rows(0x7EF, sum(counts)), counts)
    return layers, {h: [merkle.build_tree(x, h) for x in layers] for h in HEIGHTS}


def _device_trees(gpu, layers, height):
    import torch

    from vortex_amd import device as vdev, merkle

    counts = [len(x) // 32 for x in layers]
    hashes = torch.frombuffer(bytearray(b"".join(layers)), dtype=torch.uint8).to(gpu)
    before = hashes.clone()
    # the tree starts 0xFF everywhere and is followed by a guard: a row the kernel skips or a store past the end shows
    total = sum(merkle.tree_rows(c) for c in counts)
    buf = torch.full(((total + 64) * 32,), 0xFF, dtype=torch.uint8, device=gpu)
    tree, off = vdev.merkle_trees(hashes, counts, height, tree=buf[:total * 32])
    torch.cuda.synchronize()
    assert off[0] == 0 and off[-1] == total and [b - a for a, b in zip(off, off[1:])] == [merkle.tree_rows(c) for c in counts]
    assert torch.equal(hashes, before), "d_hashes was modified"
    assert bool((buf[total * 32:] == 0xFF).all()), "a store went past the tree"
    raw = buf[:total * 32].cpu().numpy().tobytes()
    return [raw[32 * a:32 * b] for a, b in zip(off, off[1:])]


@pytest.mark.parametrize("height", HEIGHTS)
def test_device_trees_every_tile_edge(built, gpu, edges, height):
    layers, want = edges
    got = _device_trees(gpu, layers, height)
    for f, (g, w) in enumerate(zip(got, want[height])):
        assert g == w, f"layer {f} of {len(layers[f]) // 32} rows at height {height}"


@pytest.mark.parametrize("height", HEIGHTS)
def test_device_trees_many_layers(built, gpu, many, height):
    layers, want = many
    got = _device_trees(gpu, layers, height)
    assert [f for f, (g, w) in enumerate(zip(got, want[height])) if g != w] == []


def test_device_trees_allocates_and_takes_a_stream(built, gpu, edges):
    import torch

    from vortex_amd import device as vdev

    layers, want = edges
    small = layers[:10]
    counts = [len(x) // 32 for x in small]
    hashes = torch.frombuffer(bytearray(b"".join(small)), dtype=torch.uint8).to(gpu)
    st = torch.cuda.Stream(device=gpu)
    st.wait_stream(torch.cuda.current_stream(gpu))
    tree, off = vdev.merkle_trees(hashes, counts, 4, stream=st)
    st.synchronize()
    assert tree.cpu().numpy().tobytes() == b"".join(want[4][:10])
    empty, off0 = vdev.merkle_trees(hashes[:0], [], 0)
    assert empty.numel() == 0 and off0 == [0]
    with pytest.raises(ValueError):
        vdev.merkle_trees(hashes, counts[:-1], 0)
    with pytest.raises(ValueError):
        vdev.merkle_trees(hashes, counts, 65)


@pytest.fixture(scope="module")
def pool(built, gpu):
    from vortex_amd.hash_pool import HashPool

    p = HashPool(16384, slots=3, slot_bytes=4 << 20)
    yield p
    p.close()


@pytest.mark.parametrize("height", HEIGHTS)
def test_build_piece_trees_every_tile_edge(pool, edges, height):
    from vortex_amd import merkle

    layers, want = edges
    st0 = pool.stats()
    trees, roots = pool.build_piece_trees(layers, PIECE_LENGTH[height])
    assert trees == want[height]
    assert roots == [t[-32:] for t in want[height]]
    assert roots[:6] == [merkle.layer_root(x, height) for x in layers[:6]]
    assert pool.stats() == st0  # leaves the statistics alone


def test_build_piece_trees_many_layers(pool, many):
    layers, want = many
    trees, roots = pool.build_piece_trees(layers, PIECE_LENGTH[4])
    assert [f for f, (g, w) in enumerate(zip(trees, want[4])) if g != w] == []
    assert roots == [t[-32:] for t in want[4]]
    assert pool.build_piece_trees([], 16384) == ([], [])
    with pytest.raises(ValueError):
        pool.build_piece_trees([b"x" * 33], 16384)


def test_build_piece_trees_while_async_pieces_are_pending(pool, edges):
    import hashlib

    layers, want = edges
    body = bytes(range(256)) * 64
    pool.spawn(0, 1, bytearray(body), len(body), hashlib.sha1(body).digest())
    trees, _ = pool.build_piece_trees(layers[:8], PIECE_LENGTH[0])  # no VX_EBUSY
    assert trees == want[0][:8]
    pool.drain()
    assert pool.try_recv().hash_matched


def _requests(rng, counts, n):
    """n random (layer, level, pos, span, uncles) requests that end at the layer's root."""
    out = []
    while len(out) < n:
        f = rng.randrange(len(counts))
        m = counts[f]
        K = (m - 1).bit_length()
        level = rng.randint(0, K)
        n_level = (m + (1 << level) - 1) >> level
        span = 1 << rng.randint(0, min(9, K - level))
        pos = rng.randrange(-(-n_level // span))
        out.append((f, level, pos, span, K - level - (span.bit_length() - 1)))
    return out


def test_proofs_from_a_device_built_tree_round_trip(pool, edges):
    """1,000 random requests answered by lookup in the trees the device built
    pass the existing verifier against the roots; with one tree row flipped the
    same proofs fail wherever they carry that row."""
    from vortex_amd import merkle

    layers, _ = edges
    height = 4
    trees, roots = pool.build_piece_trees(layers, PIECE_LENGTH[height])
    counts = [len(x) // 32 for x in layers]
    rng = random.Random(77)
    reqs = _requests(rng, counts, 1000)

    def messages(trees):
        blob, proofs, row = [], [], 0
        for f, level, pos, span, uncles in reqs:
            msg = merkle.proof_from_tree(trees[f], counts[f], height, level, pos, span, uncles)
            assert len(msg) == 32 * (span + uncles)
            blob.append(msg)
            proofs.append((pos, row, f, span, uncles))
            row += span + uncles
        return b"".join(blob), proofs

    blob, proofs = messages(trees)
    assert pool.verify_hash_proofs(blob, proofs, roots) == [True] * len(reqs)
    # a few against the host model too: the lookup is make_proof over that level's rows
    for f, level, pos, span, uncles in reqs[:20]:
        at = sum((counts[f] + (1 << k) - 1) >> k for k in range(level))
        n_level = (counts[f] + (1 << level) - 1) >> level
        want = merkle.make_proof(trees[f][32 * at:32 * (at + n_level)], height + level, pos, span, uncles)
        assert merkle.proof_from_tree(trees[f], counts[f], height, level, pos, span, uncles) == want

    # flip one row of the largest tree: a level-3 row, so proofs below and beside it carry it
    f = counts.index(262145)
    row = sum((counts[f] + (1 << k) - 1) >> k for k in range(3)) + 5
    bad = bytearray(trees[f])
    bad[32 * row + 7] ^= 0x10
    flipped = list(trees)
    flipped[f] = bytes(bad)
    reqs += [(f, 3, 5, 1, 19 - 3), (f, 3, 4, 1, 19 - 3), (f, 3, 2, 2, 19 - 4), (f, 0, 0, 1, 19)]
    blob, proofs = messages(trees)
    blob_bad, _ = messages(flipped)
    carries = [a != b for a, b in zip(_cut(blob, proofs), _cut(blob_bad, proofs))]
    assert carries[-4:] == [True, True, True, False] and sum(carries) >= 3
    got = pool.verify_hash_proofs(blob_bad, proofs, roots)
    assert got == [not c for c in carries]


def _cut(blob, proofs):
    return [blob[32 * row:32 * (row + span + uncles)] for _, row, _, span, uncles in proofs]
