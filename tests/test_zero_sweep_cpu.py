"""The zero-hash sweep's shapes (tests/_zero_sweep.py) reach every path the two
kernels can take.  Host only: the classifiers restate the kernels' arithmetic,
the reachable classes are enumerated by brute force over waves of two lengths,
and the launches of tests/test_gpu_zero_sweep.py must leave none of them out.

The hole this closes, as it stood before the sweep: the lengths a GPU had seen
(ZERO_LENS of tests/test_gpu_sparse.py for sha1_zero_kernel; 1, 55, 56, 63, 64,
16383 and 16384 for merkle_zero_leaf_kernel) have rem & 3 of 0, 1 and 3 only,
and the leaf kernel's row table and full row ran only where a test's tmp_path
reports file holes.
"""
import hashlib

import pytest

import _zero_sweep as zs

OLD_SHA1 = [1, 55, 56, 63, 64, 119, 120, 128, 16384, 65537, 262144]
OLD_LEAF = [1, 55, 56, 63, 64, 16383, 16384]
# what a classifier reads of a length: min(z, 2), rem, and (the leaf kernel) whether it is the full block
SHA1_REPS = list(range(0, 256))
LEAF_REPS = list(range(1, 256)) + [zs.LEAF]


def _sha1_reachable():
    return {zs.class_sha1(a, [a, b]) for a in SHA1_REPS for b in SHA1_REPS}


def _leaf_reachable(fulls=(False, True)):
    # (a lane below the wave's count beside a known lane takes three lengths)
    return {zs.class_leaf(a, [a, b, c], full) for full in fulls for a in LEAF_REPS for b in LEAF_REPS
            for c in (a, zs.LEAF)}


def _sha1_got(launches):
    return set().union(*(zs.classes(zs.class_sha1, lens) for _, lens in launches))


def _leaf_got(launches):
    return set().union(*(zs.classes(zs.class_leaf, lens, full) for _, lens, full in launches))


def test_constants_come_from_the_sources():
    assert (zs.SHA1_GROUP, zs.LEAF_GROUP, zs.LEAF) == (64, 256, 16384)
    assert zs.SHA1_GROUP == zs.WAVE and zs.LEAF_GROUP % zs.WAVE == 0


def test_classifiers_read_z_rem_and_full_only():
    """What lets the brute force stop at 255 bytes: a longer length is the same
    lane to both classifiers as its representative below 256."""
    for L in list(range(256, 1024)) + [4095, 65537, (1 << 20) + 57]:
        rep = 192 + (L & 63)
        for other in (0, 70, 130):
            assert zs.class_sha1(L, [L, other]) == zs.class_sha1(rep, [rep, other])
    for L in list(range(256, 1024)) + zs.LEAF_TOP[:-1]:
        rep = 192 + (L & 63)
        for other in (1, 70, 130):
            for full in (False, True):
                assert zs.class_leaf(L, [L, other], full) == zs.class_leaf(rep, [rep, other], full)
    # a full lane is known only with the row given, and then it is the wave's shortest
    assert zs.class_leaf(zs.LEAF, [zs.LEAF, 1], True) == (0, 0, False, False, True, "mixed")
    assert zs.class_leaf(zs.LEAF, [zs.LEAF, 64], True) == (0, 0, False, True, True, "mixed")
    assert zs.class_leaf(zs.LEAF, [zs.LEAF, 64], False) == (2, 0, False, False, False, "none")
    assert zs.class_leaf(zs.LEAF, [zs.LEAF], True)[5] == "all"


def test_shapes_are_the_named_ones():
    assert zs.SHA1_GRID == list(range(321)) and len(zs.SHA1_GRID) % zs.WAVE == 1
    assert sorted(zs.SHA1_SHUFFLED) == zs.SHA1_GRID and zs.SHA1_SHUFFLED != zs.SHA1_GRID
    assert all(len({L >> 6 for L in w}) > 1 for w in zs.waves_of(zs.SHA1_SHUFFLED)[:-1])
    assert zs.LEAF_GRID == list(range(1, 192)) + list(range(16384 - 65, 16385))
    assert sorted(zs.LEAF_SHUFFLED) == zs.LEAF_GRID and len(zs.LEAF_GRID) > zs.LEAF_GROUP
    for lens, lo in ((zs.SHA1_GRID, 0), (zs.LEAF_GRID, 1)):
        assert {(min(L >> 6, 2), L & 63) for L in lens} >= {(z, r) for z in range(3) for r in range(64) if 64 * z + r >= lo}
    # the long lanes: each in a wave with lanes of 0, 1, 58 and 62 bytes, which a long lane holds
    # under the select for more iterations than any length had before (4,095)
    waves = zs.waves_of(zs.SHA1_LONG)
    assert len(waves) == len(zs.SHA1_LONG_LENS) + 1 and len(waves[-1]) < zs.WAVE
    for L, w in zip(zs.SHA1_LONG_LENS, waves):
        assert w.count(L) == 1 and set(w) == {L, 0, 1, 58, 62}
    assert set(waves[-1]) == set(zs.SHA1_LONG_LENS) | {0, 1, 58, 62}
    assert max(zs.SHA1_LONG) >> 6 == 16384 and max(zs.SHA1_HUGE) >> 6 == 65536 and {0, 1, 58, 62} < set(zs.SHA1_HUGE)
    assert all(0 <= L < 1 << 29 for _, lens in zs.sha1_launches() for L in lens)
    assert all(1 <= L <= zs.LEAF for _, lens, _ in zs.leaf_launches() for L in lens)


def test_product_lanes_hold_the_three_kinds_of_wave():
    assert zs.LEAF_NS == (1, 63, 64, 65, 257, 300) and zs.leaf_lens(300) == zs.LEAF_MASTER
    w = zs.waves_of(zs.LEAF_MASTER)
    assert sorted(w[0]) == list(range(1, 64)) + [zs.LEAF]
    assert w[1] == [zs.LEAF] * 64 and zs.LEAF not in w[3] and zs.LEAF_MASTER[256] == zs.LEAF
    assert sorted(w[2]) == [zs.LEAF - 1] + [zs.LEAF] * 63
    for n in zs.LEAF_NS:
        lens = zs.leaf_lens(n)
        assert len(lens) == n and len(zs.leaf_want(lens, b"x" * 32)) == n
    kinds = {c[5] for c in zs.classes(zs.class_leaf, zs.leaf_lens(257), True)}
    assert kinds == {"all", "none", "mixed"}
    assert {c[5] for c in zs.classes(zs.class_leaf, zs.leaf_lens(63), True)} == {"none"}
    assert {c[5] for c in zs.classes(zs.class_leaf, zs.leaf_lens(65), True)} == {"mixed", "all"}


@pytest.mark.parametrize("form", zs.ROWS_FORMS)
@pytest.mark.parametrize("n", zs.LEAF_NS)
def test_row_tables_are_distinct_and_in_bounds(form, n):
    rows, out_rows = zs.rows_table(form, n)
    if form == "none":
        assert rows is None and out_rows == n
        return
    assert len(rows) == n == len(set(rows)) and 0 <= min(rows) and max(rows) < out_rows
    if form == "permuted":
        assert sorted(rows) == list(range(n)) == list(range(out_rows)) and (n < 3 or rows != sorted(rows))
    else:
        assert rows == sorted(rows) and out_rows > n and (n == 1 or max(b - a for a, b in zip(rows, rows[1:])) > 1)


def test_launches_cover_the_sha1_kernel():
    reachable = _sha1_reachable()
    zs.missing(reachable, _sha1_got(zs.sha1_launches()), "class_sha1")
    assert reachable == {(z, r, r > 55, below, False, "none") for z in range(3) for r in range(64) for below in (False, True)}
    # the lengths a GPU had seen: no rem & 3 == 2, no empty message
    old = zs.classes(zs.class_sha1, OLD_SHA1)
    assert {c[1] & 3 for c in old} == {0, 1, 3} and (0, 0, False, False, False, "none") not in old


def test_launches_cover_the_leaf_kernel():
    zs.missing(_leaf_reachable(), _leaf_got(zs.leaf_launches()), "class_leaf")
    # the public entry alone (no full row, rows = NULL) covers what can be reached without a full row
    # but the waves of one block count below 2 (the grid's start at 1 byte leaves its waves mixed),
    # which the product's n = 1 and n = 63 and a wave of the cover are
    public = _leaf_got(zs.leaf_launches()[:2])
    left = _leaf_reachable((False,)) - public
    assert left == {(z, r, r > 55, False, False, "none") for z in (0, 1) for r in range(64) if 64 * z + r not in (0, 64)}
    assert left <= zs.classes(zs.class_leaf, zs.leaf_lens(63), False) | zs.classes(zs.class_leaf, zs.LEAF_COVER, False)
    old = zs.classes(zs.class_leaf, OLD_LEAF, False)
    assert {c[1] & 3 for c in old} == {0, 1, 3} and {c[5] for c in old} == {"none"}


def test_the_coverage_check_notices_the_missing_remainders():
    """The check guards something: with the rem & 3 == 2 lengths taken out of
    the grids (each gives its lane to the length one byte below, so the waves
    stay as they are) it fails and names the missing classes, which are all
    the classes with such a remainder and no others."""
    def drop(lens):
        return [L - 1 if (L & 63) & 3 == 2 else L for L in lens]

    sha1 = [(w, drop(lens)) for w, lens in zs.sha1_launches()]
    with pytest.raises(AssertionError, match=r"class_sha1: 96 of 384 reachable classes are not covered: "
                                             r"\[\(0, 2, False, False, False, 'none'\), \(0, 2, False, True,"):
        zs.missing(_sha1_reachable(), _sha1_got(sha1), "class_sha1")
    assert _sha1_reachable() - _sha1_got(sha1) == {c for c in _sha1_reachable() if c[1] & 3 == 2}
    leaf = [(w, drop(lens), f) for w, lens, f in zs.leaf_launches()]
    with pytest.raises(AssertionError, match=r"class_leaf: \d+ of \d+ reachable classes are not covered: "
                                             r"\[\(0, 2, False, False, False, 'mixed'\)"):
        zs.missing(_leaf_reachable(), _leaf_got(leaf), "class_leaf")
    assert _leaf_reachable() - _leaf_got(leaf) == {c for c in _leaf_reachable() if c[1] & 3 == 2}
    # ... and without the cover's waves, classes of every remainder
    with pytest.raises(AssertionError, match=r"class_leaf: \d+ of \d+ reachable classes are not covered"):
        zs.missing(_leaf_reachable(), _leaf_got([x for x in zs.leaf_launches() if not x[0].startswith("cover")]),
                   "class_leaf")


def test_references_are_hashlib_once_per_length():
    zs.sha1_of_zeros.cache_clear()
    for _ in range(2):
        assert [zs.sha1_of_zeros(n) for n in (0, 2, 58)] == [hashlib.sha1(bytes(n)).digest() for n in (0, 2, 58)]
    assert zs.sha1_of_zeros.cache_info().misses == 3 and zs.sha1_of_zeros.cache_info().hits == 3
    assert zs.sha256_of_zeros(zs.LEAF) == hashlib.sha256(bytes(16384)).digest() == zs.full_row("true")
    assert zs.full_row("c3") == b"\xc3" * 32 and zs.full_row("none") is None
    want = zs.leaf_want([1, zs.LEAF, 2], zs.full_row("c3"))
    assert want == [hashlib.sha256(b"\0").digest(), b"\xc3" * 32, hashlib.sha256(b"\0\0").digest()]
    assert zs.leaf_want([zs.LEAF], None) == [hashlib.sha256(bytes(16384)).digest()]


def test_the_gpu_check_names_lane_length_and_remainders():
    """The comparison of tests/test_gpu_zero_sweep.py, fed digests that are
    wrong exactly where rem & 3 == 2 (a 0x80 one byte late): the message names
    the first lane, its length, rem and rem & 3, and the set of rem & 3."""
    import numpy as np

    from test_gpu_zero_sweep import _check_digests

    lens = zs.SHA1_SHUFFLED
    want = [zs.sha1_of_zeros(L) for L in lens]
    got = np.frombuffer(b"".join(zs.sha1_of_zeros(L + 1) if L & 3 == 2 else w for L, w in zip(lens, want)),
                        dtype=np.uint8).reshape(len(lens), 20)
    first = next(j for j, L in enumerate(lens) if L & 3 == 2)
    with pytest.raises(AssertionError, match=rf"80 of 321 digests differ from hashlib, first: lane {first} \(row {first}, "
                                             rf"len {lens[first]}, rem {lens[first] & 63}, rem & 3 = 2\); "
                                             r"rem & 3 of all: \[2\]"):
        _check_digests("model", got, lens, want)
    _check_digests("model", np.frombuffer(b"".join(want), dtype=np.uint8).reshape(len(lens), 20), lens, want)
    # through a row table: the digest of lane j is looked for in row rows[j]
    rows, out_rows = zs.rows_table("gaps", 5)
    out = np.full((out_rows, 20), 0xFF, dtype=np.uint8)
    out[rows] = np.frombuffer(b"".join(want[:5]), dtype=np.uint8).reshape(5, 20)
    _check_digests("rows", out, lens[:5], want[:5], rows)
    with pytest.raises(AssertionError, match="5 of 5 digests differ"):
        _check_digests("rows", out, lens[:5], want[:5], None if rows[0] else [r + 1 for r in rows])
