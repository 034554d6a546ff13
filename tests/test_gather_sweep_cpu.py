"""The gather sweep's shapes (tests/_gather_sweep.py) reach every path of
gather_kernel, and its model is a plain copy.  Host only: the classifiers
restate the kernel's index arithmetic, and the launches of
tests/test_gpu_gather_sweep.py must leave no class out.

The hole this closes, as it stood before the sweep: the kernel was judged by
the digests of what it copied alone, which see neither a byte written into the
gap behind a piece nor a tile copied twice, and no test chose its lengths by
the kernel's loops (the unrolled trip, the byte tail, the search over pieces
that own no tile, the stride loop above the grid cap).
"""
import math

import numpy as np
import pytest

import _gather_sweep as gs


def test_constants_come_from_the_source():
    assert (gs.TILE, gs.BLOCK, gs.GRID, gs.U) == (65536, 256, 64, 4)
    assert gs.TRIP == 1024 and gs.FULL == 4096 and gs.FULL % gs.TRIP == 0 and gs.FULL > 2 * gs.TRIP
    with pytest.raises(RuntimeError, match="expected one definition of kNoSuchDepth"):
        gs._constants(gs.os.path.join(gs._CSRC, "vx_gather.hip"), ("kNoSuchDepth",))


def test_no_class_is_left_out():
    got = gs.covered()
    assert gs.missing(got) == []
    assert got["words"] == set(gs.WORD_CLASSES) and got["tail"] == set(gs.TAIL_CLASSES)
    assert got["piece"] == set(gs.PIECE_CLASSES) and got["n"] == set(gs.N_CLASSES)
    assert got["tileless"] == set(gs.TILELESS_AT)
    assert all(got["grid"][g] == set(gs.GRID_CLASSES) for g in gs.MAX_GRIDS) and set(got["grid"]) == {0, 1, 128}
    # a full tile has no tail; every other class of words meets every class of tail
    assert {t for w, t in got["tile"] if w == "full tile"} == {"0"}
    # the one list alone reaches every class of tile and of piece, and every place of a tileless piece
    cover = gs.covered({"cover": gs.SHAPES["cover"]})
    assert [m for m in gs.missing(cover) if not m.startswith(("n ", "max_grid"))] == []


def test_the_coverage_check_notices_what_is_missing():
    """The check guards something: without the tails of 15 bytes, without the
    table of nine pieces or without the tables built for the grid caps it
    names exactly what is gone."""
    no15 = {k: [(L - 1 if L % 16 == 15 else L, g) for L, g in s] for k, s in gs.SHAPES.items()}
    left = gs.missing(gs.covered(no15))
    assert "tail 15" in left and all("15" in m for m in left) and len(left) == 1 + len(gs.WORD_CLASSES) - 1
    no9 = {k: s for k, s in gs.SHAPES.items() if len(s) != 9}
    assert gs.missing(gs.covered(no9)) == ["n 2^k+1"]
    few = {k: s for k, s in gs.SHAPES.items() if not k.startswith("tiles")}
    left = gs.missing(gs.covered(few))
    assert left and all(m.startswith("max_grid") for m in left)
    assert "max_grid 128: ntiles twice and one the cap" in left and "max_grid 0: ntiles equal the cap" in left
    # without pieces the launch does not gather
    allg = {k: [(L, True) for L, g in s] for k, s in gs.SHAPES.items()}
    assert "piece 0: not gathered" in gs.missing(gs.covered(allg))


def test_the_cover_list_is_the_small_one():
    shape = gs.SHAPES["cover"]
    lay = gs.layout("cover")
    assert lay.ntiles == 2 * gs.GRID + 1 == 129 and 60 <= len(shape) <= 100
    assert sum(L for L, g in shape if g) < 6 << 20 and lay.arena_bytes < 8 << 20
    assert all(L < 1 << 22 for s in gs.SHAPES.values() for L, g in s)  # far from the lengths at which gather_tiles wrapped
    assert sorted(gs.layout(k).ntiles for k in gs.SHAPES if k.startswith("tiles")) == [0, 1, 2, 3, 63, 64, 65, 127, 128,
                                                                                      129, 257]
    assert all(gs.layout(k).arena_bytes < 8 << 20 for k in gs.SHAPES)
    assert sorted({len(s) for k, s in gs.SHAPES.items() if k.startswith("n")}) == [1, 2, 3, 7, 8, 9]


@pytest.mark.parametrize("name", list(gs.SHAPES))
def test_tfirst_is_the_ceiling_over_gathered_pieces(name):
    lay = gs.layout(name)
    acc, want = 0, [0]
    for L, g in lay.shape:
        acc += math.ceil(L / gs.TILE) if g else 0
        want.append(acc)
    assert lay.tfirst == want and lay.ntiles == want[-1] and len(lay.tfirst) == lay.n + 1
    # the kernel's search, step for step, finds the owner of every tile: pieces that own none are never chosen
    owner = [i for i, (L, g) in enumerate(lay.shape) for _ in range(gs.tiles_of(L) if g else 0)]
    assert [gs.search(lay.tfirst, lay.n, t) for t in range(lay.ntiles)] == owner
    assert all(lay.gathered[i] and lay.lens[i] for i in owner)


@pytest.mark.parametrize("name", list(gs.SHAPES))
def test_layouts_are_what_the_kernel_is_promised(name):
    lay = gs.layout(name)
    n = lay.n
    spans = sorted((lay.dst[i], lay.dst[i] + lay.lens[i]) for i in range(n))
    assert all(d % 16 == 0 for d, _ in spans)
    assert spans[0][0] == gs.SLACK and lay.arena_bytes - spans[-1][1] >= gs.SLACK
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert 16 <= b0 - (a1 + 15) // 16 * 16 <= 272, "destinations are 16 to 272 bytes apart"
    if name in gs.DESCENDING:
        assert lay.dst == sorted(lay.dst, reverse=True) and n > 1
    elif n > 3:
        assert lay.dst != sorted(lay.dst) and lay.dst != sorted(lay.dst, reverse=True)
    live = [i for i in range(n) if lay.gathered[i]]
    assert all(lay.src[i] >= 0 and lay.src[i] % 16 == 0 and lay.src[i] + lay.lens[i] <= lay.src_bytes for i in live)
    assert all(lay.src[i] == -1 for i in range(n) if not lay.gathered[i])
    assert lay.data.size == lay.src_bytes and not (lay.data == gs.FILL).any()
    if any(lay.lens[i] for i in live):
        assert max(lay.src[i] + lay.lens[i] for i in live) == lay.src_bytes, "a source ends on the last byte"
    src, dst, lens, tfirst = lay.tables(0x7000_0000_0000)
    assert src.dtype == dst.dtype == np.uint64 and lens.dtype == tfirst.dtype == np.uint32
    assert [int(s) for s in src] == [0x7000_0000_0000 + s if s >= 0 else 0 for s in lay.src]


def test_sources_are_shared_and_unrelated_to_the_destinations():
    lay = gs.layout("cover")
    a, b = lay.shared
    assert a != b and lay.src[a] == lay.src[b] and 16 <= lay.lens[a] <= lay.lens[b]
    live = [i for i in range(lay.n) if lay.gathered[i] and lay.lens[i] and i != a]
    by_src, by_dst = sorted(live, key=lambda i: lay.src[i]), sorted(live, key=lambda i: lay.dst[i])
    assert by_src != by_dst and by_src != by_dst[::-1]
    assert sum(1 for k in gs.SHAPES if gs.layout(k).shared) >= 10


def test_model_is_a_byte_by_byte_copy():
    for name in ("n9", "n7", "tiles 3"):
        lay = gs.layout(name)
        want = bytearray([gs.FILL]) * lay.arena_bytes
        for i in range(lay.n):
            if lay.shape[i][1]:
                for k in range(lay.lens[i]):
                    want[lay.dst[i] + k] = int(lay.data[lay.src[i] + k])
        got = gs.model(lay)
        assert got.dtype == np.uint8 and got.tobytes() == bytes(want)
        assert got.tobytes() != bytes([gs.FILL]) * lay.arena_bytes
    lay = gs.layout("tiles 0")
    assert lay.ntiles == 0 and (gs.model(lay) == gs.FILL).all()


def test_the_message_names_piece_tile_offset_and_class():
    lay = gs.layout("n9")
    want = gs.model(lay)
    assert gs.first_difference(lay, want.copy(), want) is None
    got = want.copy()
    i = 4  # 5 tiles
    got[lay.dst[i] + 3 * gs.TILE + 77] ^= 1
    msg = gs.first_difference(lay, got, want)
    assert f"piece 4 (len {5 * gs.TILE}, 5 tiles), tile 3 of the piece (tile {lay.tfirst[4] + 3} of {lay.ntiles}), " \
           "offset 77 within the tile, class: words full tile, tail 0" in msg and msg.startswith("n9: 1 arena bytes")
    got = want.copy()
    got[lay.dst[6] + lay.lens[6] + 2] = 0  # an over-copy into the gap behind a piece of 47 bytes
    msg = gs.first_difference(lay, got, want)
    assert "no destination: 2 bytes past the end of piece 6 (len 47, gathered True)" in msg
    assert "offset 49 within it, class: words <block, tail 15" in msg
    got = want.copy()
    got[lay.dst[2] + 10] = 1  # the piece the launch does not gather
    assert "piece 2 (len 50), which is not gathered: byte 10" in gs.first_difference(lay, got, want)
    got = want.copy()
    got[5] = 0
    assert "the slack in front" in gs.first_difference(lay, got, want)
