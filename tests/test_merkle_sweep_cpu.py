"""CPU: the merkle sweep's shapes (tests/_merkle_sweep.py) leave no class of
lane, wave, tile position or width out, shown by brute force from the lengths
and widths alone; the check itself fails, naming the class, when the shapes
are doctored; the model agrees with a plain recursion; hashlib is quick enough
for all of it.  No GPU, no library."""
import hashlib
import time

import pytest

import _merkle_sweep as sw


# ---------------------------------------------------------------------------
# the leaf lanes
# ---------------------------------------------------------------------------
def test_constants_and_grid():
    assert sw.LEAF == 16384 and sw.GROUP == 256 and sw.RING == 2
    assert (1 << sw.TILE_LOG2, 1 << sw.PIECE_TILE_LOG2) == (512, 256)
    assert sw.GRID == [128 * g + r for g in (0, 1, 2, 3, 126, 127) for r in range(128)] + [16384]
    assert {(L & 127) % 4 for L in sw.GRID} == {0, 1, 2, 3}


def test_recipes_are_the_named_waves():
    rec = sw.recipes()
    ng = {name: [L >> 7 for L in w] for name, w in rec.items()}
    for g in (0, 1, 2, 3, 4, 5, 6, 125, 126, 127, 128):
        assert set(ng[f"uniform {g}"]) == {g}
    for g in (128, 127, 5, 4):
        for lane in (0, 63, 31):
            w = ng[f"{sw.MIXED}one lane of {g} groups at lane {lane}"]
            assert w[lane] == g and {x for k, x in enumerate(w) if k != lane} == {0, 1, 2}
    assert ng[sw.MIXED + "ascending"] == list(range(64)) == ng[sw.MIXED + "descending"][::-1]
    assert rec["all empty"] == [0] * 64
    assert all(0 < L < 128 for L in rec["all tails below a group"])
    w = rec[sw.MIXED + "full leaves and one empty lane"]
    assert sorted(w) == [0] + [sw.LEAF] * 63
    for g in (0, 1, 2, 127):
        both = rec[f"tails 0..63 at {g} groups"] + rec[f"tails 64..127 at {g} groups"]
        assert both == [128 * g + r for r in range(128)]
    # what carries the prefix is what mixes group counts, and nothing else does
    for name, w in ng.items():
        assert (len(set(w)) > 1) == name.startswith(sw.MIXED), name


def test_batch_size_and_last_row():
    lens = sw.leaf_batch()
    n = len(lens)
    assert n % 64 and n % 256 and n > 64 * len(sw.recipes())
    assert 0 < lens[-1] < sw.LEAF and (lens[-1] & 127) % 4 == 2  # the row the lanes past the end redo
    assert sum(lens) < 16 << 20
    for at, part, skipped in sw.blocks_launches(lens):
        assert len(part) * sw.LEAF < 16 << 20 and at % 64 == 0
    assert any(len(part) % 64 for _, part, _ in sw.blocks_launches(lens))


def test_uniform_pairs():
    pairs = sw.uniform_pairs()
    walk = [p for p in pairs if not p[0].startswith(sw.MIXED)]
    assert len(walk) * 10 >= len(sw.GRID) and all(n == 65 for _, _, _, n in walk)
    for name, a, b, n in pairs:
        assert 0 < b <= a <= sw.LEAF, name  # what vx_merkle_device_uniform accepts
        s = sw.uniform_stride(a)
        assert s % 16 == 0 and s % 128 and s >= a
    classes = lambda L: frozenset(sw.lane_classes(L))
    assert all(classes(a) != classes(b) or a == 1 for _, a, b, _ in walk)  # another tail class each time
    assert len({b for _, _, b, _ in walk}) > len(walk) // 2


def test_every_leaf_class_in_every_entry():
    launches = sw.leaf_launches()
    assert set(launches) == set(sw.ENTRIES) and len(sw.ENTRIES) == 5
    sw.check_leaf_cover(launches)
    # the classes are those of the kernel's own arithmetic: every length of a leaf falls in some
    for L in range(sw.LEAF + 1):
        c = sw.lane_classes(L)
        assert c and c <= set(sw.LANE_CLASSES)
    assert set().union(*(sw.lane_classes(L) for L in range(sw.LEAF + 1))) == set(sw.LANE_CLASSES)


def test_cover_check_fails_without_two_byte_partial_words():
    """Every length with rem % 4 == 2 replaced by its neighbour: no such length is left."""
    fix = lambda L: L + 1 if L < sw.LEAF and (L & 127) % 4 == 2 else L
    doctored = sw.leaf_launches(fix=fix)
    assert not any((L & 127) % 4 == 2 and L < sw.LEAF for launches in doctored.values() for la in launches for L in la)
    with pytest.raises(AssertionError, match=r"rem % 4 == 2"):
        sw.check_leaf_cover(doctored)


def test_cover_check_fails_without_mixed_waves():
    doctored = sw.leaf_launches(keep=lambda name: not name.startswith(sw.MIXED))
    with pytest.raises(AssertionError, match=r"0 < ng < ng_wave"):
        sw.check_leaf_cover(doctored)
    with pytest.raises(AssertionError, match=r"the one longest lane is lane 0"):
        sw.check_leaf_cover(doctored)


def test_layout_phases_and_gaps():
    lens = sw.leaf_batch()
    offs, host, flipped = sw.layout(lens)
    assert all(o % 16 == 0 for o in offs)
    assert all((o // 16) % 8 == i % 8 for i, o in enumerate(offs))
    assert {(o // 16) % 8 for o in offs} == set(range(8))
    ends = [o + L for o, L in zip(offs, lens)]
    assert all(offs[i + 1] - ends[i] >= 16 for i in range(len(lens) - 1)) and len(host) - ends[-1] >= 64
    assert len(host) < 16 << 20
    gaps = b"".join(host[ends[i]:offs[i + 1]].tobytes() for i in range(len(lens) - 1))
    assert len(set(gaps)) == 256  # random, not a fill
    for o, L in zip(offs[:200], lens[:200]):
        assert (flipped[o:o + L] == host[o:o + L]).all()
        assert (flipped[o + L:o + L + 16] == host[o + L:o + L + 16] ^ 0xFF).all()


# ---------------------------------------------------------------------------
# the tree shapes
# ---------------------------------------------------------------------------
SHAPES = [(kern, K) for kern, top in sw.KERNELS.items() for K in range(top + 1)]


@pytest.mark.parametrize("kernel,K", SHAPES)
def test_tree_shape_reaches_every_position_and_width(kernel, K):
    per = sw.per_tile(kernel, K)
    assert per == ((512 if kernel == "node" else 256) >> K)
    lw = sw.tree_shape(kernel, K)
    n = len(lw)
    sw.check_tree_cover(kernel, K, lw)
    assert (n - 1) % per == 0 and (n - 1) // per >= 2 and n >= 2 * (K + 1)
    # by hand, not through tree_classes
    for w in range(K + 1):
        assert any(lw[i] == w and i % per == 0 and i + per <= n for i in range(n)), f"width {w} at position 0"
        assert any(lw[i] == w and i % per == per - 1 for i in range(n)), f"width {w} at position per - 1"
    if kernel == "node" and K == 0:
        assert any(i % 512 < 256 for i in range(n)) and any(i % 512 >= 256 for i in range(n))
    assert sw.count_batches(kernel, K) == sorted({x for x in (1, per - 1, per, per + 1) if x > 0})
    # the check notices a width that is missing at a tile's edge
    if K:
        doctored = [w if i % per not in (0, per - 1) or w != K else 0 for i, w in enumerate(lw)]
        with pytest.raises(AssertionError, match=r"not reached"):
            sw.check_tree_cover(kernel, K, doctored)


@pytest.mark.parametrize("K", sw.WIDE)
def test_wide_shape(K):
    shape = sw.wide_shape(K)
    ws = [w for w, _ in shape]
    assert sorted(ws[:-1]) == list(range(K + 1)) and ws[0] != K and ws[-1] == K
    assert shape[-1][1] == 256 * 16384 + 1
    assert (K, 16384 << K) in shape  # the widest piece is whole: every tile's top is a real hash
    assert all(L <= 16384 << w for w, L in shape)


def _plain_root(data, w):
    """The root of a piece of width w, recursively, from the bytes."""
    def node(lo, count):
        if count == 1:
            at = lo * 16384
            return hashlib.sha256(data[at:at + 16384]).digest() if at < len(data) else bytes(32)
        return hashlib.sha256(node(lo, count // 2) + node(lo + count // 2, count // 2)).digest()

    return node(0, 1 << w)


def test_model_against_a_plain_recursion():
    data = sw.random_bytes(1, 16384 << 5).tobytes()
    for w, L in ((0, 16384), (3, 16384 << 3), (5, 16384 << 5), (5, (16384 << 4) + 1), (4, 16384 * 7 + 130), (0, 77)):
        assert sw.tree_root(sw.leaf_rows(data[:L], w)) == _plain_root(data[:L], w), (w, L)
    for w in (0, 1, 6):
        assert sw.tree_root(sw.leaf_rows(b"", w)) == sw.pad_hash(w) == _plain_root(b"", w)
    rows = [bytes([k]) * 32 for k in range(5)]
    padded = rows + [sw.pad_hash(0)] * 3
    assert sw.layer_root(rows) == sw.tree_root(padded)


def test_piece_batch_model():
    """A small width end to end: an empty piece's root is the pad hash of its
    own width, a half piece's upper leaves are zero rows."""
    b = sw.piece_batch(2)
    view = memoryview(b.host)
    seen = set()
    for i, (o, L, w) in enumerate(zip(b.offs, b.lens, b.lw)):
        assert b.roots[i].tobytes() == _plain_root(view[o:o + L].tobytes(), w)
        if L == 0:
            assert b.roots[i].tobytes() == sw.pad_hash(w)
        seen.add("empty" if L == 0 else "whole" if L == 16384 << w else "half")
        assert (b.leaves[(i << 2) + (1 << w):(i + 1) << 2] == 0).all()
    assert seen == {"empty", "whole", "half"}


def test_references_build_quickly():
    """Everything the GPU files compare against, built once here: a few seconds at the most."""
    t0 = time.perf_counter()
    lens = sw.leaf_batch()
    offs, host, _ = sw.layout(lens)
    sw.hash_rows(host, offs, lens)
    nodes = 0
    for K in range(sw.TILE_LOG2 + 1):
        lw = sw.tree_shape("node", K)
        sw.node_rows(K, lw)
        nodes += sum((1 << w) - 1 for w in lw)
    assert nodes < 10000  # a few thousand node hashes: K + 1 or more tiles a width
    total = 0
    for K in list(range(sw.PIECE_TILE_LOG2 + 1)) + list(sw.WIDE):
        total += sum(sw.piece_batch(K).lens)
    took = time.perf_counter() - t0
    print(f"leaf batch {sum(lens) >> 20} MiB, piece batches {total >> 20} MiB, {nodes} node hashes: {took:.2f} s")
    assert took < 10
