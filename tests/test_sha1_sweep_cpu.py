"""The SHA-1 sweep's shapes (tests/_sha1_sweep.py) reach every path the
kernels' loops can take.  Host only: the classifiers restate the kernels' index
arithmetic, the reachable classes are enumerated by brute force, and the grid
and the wave recipes must leave none of them out.  tests/test_gpu_sha1_sweep.py
runs these shapes on the device against hashlib.

The hole this closes, as it stood before the sweep: the lengths of
test_uniform_lengths_vs_oracle (1, 55, 56, 64, 127, 128, 129, 4096, 65556,
262144; the only test pinning uniform variants 1 and 2) have group counts
ng = len >> 7 of 0, 0, 0, 0, 0, 1, 1, 32, 512, 2048.  Once ng >= kLaneRing = 4
they reach only ng % kLaneRing == 0 (the fenced loop's remainder never runs
after a full trip), and once ng >= kRing = 3 only ng % kRing == 2; none has an
odd trailing block after a streamed ring, and nb % 6 is never 0 or 4.
"""
import ctypes

import pytest

import _sha1_sweep as sw

# every full-block count a length below 4096 can have, with the four kinds of
# tail that the kernels tell apart (none, the longest with one padding block,
# the shortest and the longest with two): the wave classifiers read a length
# only through nfull and rem > 55 (test_wave_classifiers_read_nfull_and_pad_only)
TWO_LENGTH_REPS = [64 * f + r for f in range(64) for r in (0, 55, 56, 63)]


def _missing(reachable, got, what):
    left = sorted(reachable - got)
    assert not left, f"{what}: {len(left)} of {len(reachable)} reachable classes are not covered: {left}"
    assert got <= reachable, f"{what}: classes outside the brute-force set: {sorted(got - reachable)}"


def test_constants_come_from_the_sources():
    assert min(sw.kRing, sw.kLaneRing, sw.kBlockRing, sw.kZcTileBlocks) >= 2 and sw.kSplitSlots in (2, 3)
    assert sw.kZcPieces * 2 == sw.WAVE  # lanes 32-63 of a zero-copy pair mirror lanes 0-31
    assert sw.kAsmUnroll % sw.kSplitSlots == 0 and sw.kAsmUnroll % 2 == 0  # slots cycle by 3, word sets by 2
    with pytest.raises(RuntimeError, match="kNoSuchRing"):
        sw._constants(sw.os.path.join(sw._CSRC, "vx_kernels.h"), ("kNoSuchRing",))


def test_grid_spans_two_trips_of_every_loop_and_its_remainders():
    assert sw.GRID == [64 * f + r for f in range(sw.GRID_BLOCKS + 1) for r in sw.TAILS]
    assert len(set(sw.GRID)) == len(sw.GRID) == (sw.GRID_BLOCKS + 1) * 11
    for blocks_per_trip in (2 * sw.kLaneRing, 2 * sw.kRing, sw.kBlockRing, sw.kAsmUnroll, 2 * sw.kZcTileBlocks):
        assert sw.GRID_BLOCKS >= 3 * blocks_per_trip
    if sw._TRIP == 16:
        assert len(sw.GRID) == 539 and max(sw.GRID) == 3135


def test_grid_covers_the_uniform_kernels():
    lengths = range(4096)
    _missing({sw.class_uniform_lane(L) for L in lengths}, {sw.class_uniform_lane(L) for L in sw.GRID}, "uniform lane")
    # the full product: every trip count with every remainder and both parities
    assert {sw.class_uniform_lane(L) for L in sw.GRID} >= {(t, m, o) for t in (1, 2) for m in range(sw.kLaneRing)
                                                            for o in (0, 1)}
    for slots in (2, 3):
        _missing({sw.class_uniform_split(L, slots) for L in lengths},
                 {sw.class_uniform_split(L, slots) for L in sw.GRID}, f"uniform split, {slots} slots")
    got = {sw.class_uniform_split(L)[:3] for L in sw.GRID}
    assert got >= {(t, m, o) for t in (1, 2) for m in range(sw.kRing) for o in (0, 1)}
    assert {sw.class_uniform_split(L)[3:] for L in sw.GRID} == {(k, p) for k in range(sw.kAsmUnroll)
                                                               for p in (False, True)}


def test_wave_classifiers_read_nfull_and_pad_only():
    """What lets the brute force over two-length waves use four tails per
    block count: two lengths with the same nfull and the same number of
    padding blocks are the same lane to every wave classifier."""
    other = 64 * 7 + 56
    for L in range(4096):
        rep = (L & ~63) + (56 if (L & 63) > 55 else 0)
        for fn in (sw.class_ragged_lane, sw.class_ragged_split, sw.class_zero_copy):
            assert fn([L, other]) == fn([rep, other]) and fn([L]) == fn([rep])


@pytest.mark.parametrize("width", [sw.WAVE, sw.kZcPieces])
def test_recipes_cover_the_wave_kernels(width):
    """Lane order: 64 consecutive lanes of a ragged launch, or the 32 pieces of
    a zero-copy pair, over both batches the GPU sweep launches."""
    main, shuffled = sw.batch_waves(width), sw.batch_s()
    assert len(main) % width == 1 and len(shuffled) % width  # T: a last wave of one live lane; S ends partial too
    waves = sw.waves_of(main, width) + sw.waves_of(shuffled, width)
    for fn in sw.wave_classifiers(width):
        reachable = {fn([a, b]) for a in TWO_LENGTH_REPS for b in TWO_LENGTH_REPS}
        _missing(reachable, {fn(w) for w in waves if len(set(w)) <= 2}, fn.__name__)


def test_the_coverage_check_notices_a_dropped_recipe():
    """The check above guards something: without recipe M (and the cover C,
    which is built from what H and M leave out) it fails and names the missing
    classes, and so does the grid without its odd group counts."""
    h_only = sw.waves_of(sw.flatten(sw.recipe_h()), sw.WAVE) + sw.waves_of(sw.batch_s())
    reachable = {sw.class_ragged_split([a, b]) for a in TWO_LENGTH_REPS for b in TWO_LENGTH_REPS}
    with pytest.raises(AssertionError, match=r"class_ragged_split: \d+ of \d+ reachable classes are not covered: \[\("):
        _missing(reachable, {sw.class_ragged_split(w) for w in h_only if len(set(w)) <= 2}, "class_ragged_split")
    even = [L for L in sw.GRID if (L >> 7) % 2 == 0]
    with pytest.raises(AssertionError, match=r"uniform lane: \d+ of \d+ reachable classes are not covered"):
        _missing({sw.class_uniform_lane(L) for L in range(4096)}, {sw.class_uniform_lane(L) for L in even},
                 "uniform lane")
    # C adds nothing that H and M already reach, and every wave of it is needed
    for width in (sw.WAVE, sw.kZcPieces):
        have = [{fn(w) for w in sw.recipe_h(width) + sw.recipe_m(width)} for fn in sw.wave_classifiers(width)]
        for w in sw.recipe_c(width):
            new = [fn(w) not in seen for fn, seen in zip(sw.wave_classifiers(width), have)]
            assert any(new), w
            for fn, seen in zip(sw.wave_classifiers(width), have):
                seen.add(fn(w))


def test_h_and_m_reach_all_nine_phase_combinations():
    """Phase 1 trips (0, 1, more) x phase 2 trips (1, 2, more) of the ragged
    split kernel, from recipes H and M alone; and the edges the old lengths
    never met: phase 2 holding only padding, and a longest lane whose second
    padding block lies one block past the others."""
    classes = {sw.class_ragged_split(w) for w in sw.recipe_h() + sw.recipe_m()}
    assert {c[:2] for c in classes} == {(a, b) for a in (0, 1, 2) for b in (1, 2, 3)}
    assert any(c[0] >= 1 and c[2] for c in classes)
    assert [64 * 6 + 0] * 63 + [64 * 6 + 63] in [sorted(w) for w in sw.recipe_m()]


# ---------------------------------------------------------------------------
# The resumable chunk kernel: lanes are (length, final)
# ---------------------------------------------------------------------------
def _chunk_reachable():
    """Every class a wave of two kinds of lane can take, nfull 0..63."""
    kinds = sw.CHUNK_KINDS
    return {sw.class_chunk([a, b]) for i, a in enumerate(kinds) for b in kinds[i:]}


def _chunk_classes(recipes):
    waves = [w for r in recipes for w in sw.waves_of(sw.chunk_batch(r))]
    return {sw.class_chunk(w) for w in waves if len(set(w)) <= 2}


def test_chunk_classifier_reads_nfull_pad_and_final_only():
    """What lets the brute force use four tails per block count: as
    test_wave_classifiers_read_nfull_and_pad_only, for the final lanes."""
    others = [(64 * 7 + 56, True), (64 * 9, False)]
    for L in range(4096):
        rep = (L & ~63) + (56 if (L & 63) > 55 else 0)
        for o in others:
            assert sw.class_chunk([(L, True), o]) == sw.class_chunk([(rep, True), o])
    with pytest.raises(AssertionError):
        sw.class_chunk([(100, False)])  # a lane that does not end its piece is whole blocks
    with pytest.raises(AssertionError):
        sw.class_chunk([(0, False)])


def test_chunk_recipes_cover_the_chunk_kernel():
    """Every class that a wave of two kinds of lane can take is taken by a wave
    the GPU sweep launches (tests/test_gpu_sha1_chunk_sweep.py runs every
    recipe's batch)."""
    reachable = _chunk_reachable()
    _missing(reachable, _chunk_classes(sw.CHUNK_RECIPES), "class_chunk")
    for r in sw.CHUNK_RECIPES:
        assert len(sw.chunk_batch(r)) % sw.WAVE == 1  # a last wave of one live lane
    # the holes the sweep is there for: a wave without phase 2 after zero, one and more
    # trips of phase 1 cannot exist (b1 == nb_wave > 0 needs a trip), after one and more it does;
    # every nfull % kBlockRing of whole-block lanes; a final lane among whole-block lanes
    got = _chunk_classes(sw.CHUNK_RECIPES)
    assert {c[0] for c in got if c[2]} == {1, 2} and all(c[1] == 0 and c[4] and not c[3] for c in got if c[2])
    whole = {x[0] >> 6 for w in sw.chunk_waves("whole") for x in w}
    assert {f % sw.kBlockRing for f in whole} == set(range(sw.kBlockRing))
    assert any(c[4] and c[5] and c[6] for c in got)


def test_the_chunk_coverage_check_notices_a_dropped_recipe():
    """Without the mixed recipes (and the cover, which is built from what the
    recipes leave out) the check fails and names the missing classes; and every
    wave of the cover is needed."""
    reachable = _chunk_reachable()
    with pytest.raises(AssertionError, match=r"class_chunk: \d+ of \d+ reachable classes are not covered: \[\("):
        _missing(reachable, _chunk_classes(("final", "whole")), "class_chunk")
    with pytest.raises(AssertionError, match=r"class_chunk: \d+ of \d+ reachable classes are not covered: \[\("):
        _missing(reachable, _chunk_classes(sw.CHUNK_RECIPES[:-1]), "class_chunk")
    seen = {sw.class_chunk(w) for r in sw.CHUNK_RECIPES[:-1] for w in sw.chunk_waves(r)}
    for w in sw.chunk_cover():
        assert sw.class_chunk(w) not in seen, w
        seen.add(sw.class_chunk(w))


def test_chain_plan_cuts_every_grid_piece_at_the_ring_edges():
    plan = sw.chain_plan()
    assert [L for L, _ in plan] == [L for L in sw.GRID if L > 64]
    used = set()
    for L, chunks in plan:
        assert 2 <= len(chunks) <= 4 and sum(chunks) == L and chunks[-1] > 0
        assert all(c % 64 == 0 and c >> 6 in sw.CHAIN_CUTS for c in chunks[:-1])
        used.update(c >> 6 for c in chunks[:-1])
    assert used == set(sw.CHAIN_CUTS)
    assert any(chunks[-1] == 64 for _, chunks in plan) and any(chunks[-1] < 56 for _, chunks in plan)
    assert {len(chunks) for _, chunks in plan} == {2, 3, 4}


def _schedule(L, C, head, tail):
    from vortex_amd import _lib

    fn = _lib.tuning().vx_tuning_chunk_schedule
    n = fn(L, C, head, tail, None, 0)
    out = (ctypes.c_uint64 * (2 * max(n, 1)))()
    assert fn(L, C, head, tail, out, n) == n
    return [(out[2 * i], out[2 * i + 1]) for i in range(n)]


CHUNK_MULTIPLE_CASES = [(chunk, ramp, pl) for chunk in (12288, 24576) for ramp in (0, 1, 5)
                        for pl in (294912, 300000, 294912 + 56)]


@pytest.mark.parametrize("chunk,ramp,pl", CHUNK_MULTIPLE_CASES)
def test_chunk_cases_have_rounds_of_whole_rings(built, chunk, ramp, pl):
    """tests/test_gpu_chunk_multiples.py: a wave of non-final chunks whose
    block count is a multiple of kBlockRing has b1 == nb_wave, so the chunk
    kernel skips phase 2 altogether.  Every schedule the re-verify can form for
    these cases (first, middle and last window) has such rounds."""
    ring_bytes = 64 * sw.kBlockRing
    assert chunk % ring_bytes == 0
    for head, tail in ((ramp, ramp), (ramp, 0), (0, ramp), (0, 0)):
        rounds = _schedule(pl, chunk, head, tail)
        assert sum(ln for _, ln in rounds) == pl
        whole = [ln for _, ln in rounds[:-1] if ln % ring_bytes == 0]
        assert whole and chunk in whole, (head, tail, rounds)
    plain = _schedule(pl, chunk, 0, 0)
    if pl % chunk == 0:  # the final chunk is a whole chunk: its only phase 2 block is padding
        assert plain[-1][1] == chunk
    # the host batches' rounds are plain chunks (round k: bytes [k*C, (k+1)*C))
    assert plain == [(a, min(chunk, pl - a)) for a in range(0, pl, chunk)]
