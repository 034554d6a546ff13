"""GPU: the files calls that keep and check the 16 KiB leaf layer
(HashPool.hash_merkle_files_leaves, HashPool.verify_merkle_files_blocks)
against hashlib: the leaf table, the bad-block bitmap, layer_ok and the bad
counts.  The pool's rounds hold 16 blocks, so they cut mid-piece and the small
files' groups are narrower than the call."""
import ctypes
import hashlib
import os
import random

import pytest

from _sparse import NO_HOLES, holes_reported, make_file

pytestmark = pytest.mark.gpu
BLOCK = 16384
MiB = 1 << 20

# per piece length: files whose pieces cover full pieces, a short last piece, one-block and tiny files
TORRENTS = {
    16384: [1, BLOCK, BLOCK + 1, 5 * BLOCK + 7, 0, 40000],
    65536: [200000, 1, 65537, 100000, 0, 3 * BLOCK, BLOCK],
    MiB: [2 * MiB + 5 * BLOCK + 9, 7, BLOCK, 3 * BLOCK, MiB + 1],
    # pieces: 0, 1 full | 2: 71 blocks | 3: the one-block file | 4: two blocks | 5: one byte
    2 * MiB: [4 * MiB + 70 * BLOCK + 100, BLOCK, 20000, 1],
}


def rand(seed, n):
    return random.Random(seed).randbytes(n)


def write_files(root, datas):
    paths = []
    for k, d in enumerate(datas):
        paths.append(str(root / f"f{k}"))
        with open(paths[-1], "wb") as f:
            f.write(d)
    return paths


def flip(path, at):
    with open(path, "r+b") as f:
        f.seek(at)
        b = f.read(1)
        f.seek(at)
        f.write(bytes([b[0] ^ 0x40]))


class Torrent:
    """Files on disk and their hashlib tables, computed once."""

    def __init__(self, root, flens, pl, seed=0):
        from vortex_amd import merkle

        self.pl, self.flens = pl, flens
        self.datas = [rand(seed + 31 * k, n) for k, n in enumerate(flens)]
        self.paths = write_files(root, self.datas)
        self.lens, self.log2w, self.findex, self.foff = merkle.torrent_pieces(flens, pl)
        self.n = len(self.lens)
        self.first, self.blocks, self.rows = merkle.leaf_layout(flens, pl)
        self.table = merkle.file_leaf_table(self.paths, flens, pl)
        self.roots = b"".join(self.root_of(self.leaves(i), self.log2w[i]) for i in range(self.n))
        self.wpp = max(1, pl // BLOCK // 64)

    def piece(self, i, datas=None):
        d = (datas or self.datas)[self.findex[i]]
        return d[self.foff[i]:self.foff[i] + self.lens[i]]

    def leaves(self, i, table=None):
        return (table or self.table)[32 * self.first[i]:32 * (self.first[i] + self.blocks[i])]

    @staticmethod
    def root_of(rows, lw):
        rows = [rows[k:k + 32] for k in range(0, len(rows), 32)]
        rows += [bytes(32)] * ((1 << lw) - len(rows))
        while len(rows) > 1:
            rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
        return rows[0]

    def words(self, bad_lists, first=0, count=None):
        """The bitmap of pieces [first, first + count) from per-piece block lists."""
        count = self.n - first if count is None else count
        out = [0] * (count * self.wpp)
        for i in range(first, first + count):
            for b in bad_lists.get(i, ()):
                out[(i - first) * self.wpp + (b >> 6)] |= 1 << (b & 63)
        return out


@pytest.fixture(scope="module")
def pool(built, gpu):
    from vortex_amd.hash_pool import HashPool

    p = HashPool(16384, slots=3, slot_bytes=262144)
    yield p
    p.close()


@pytest.fixture(scope="module")
def torrents(tmp_path_factory):
    made = {}

    def get(pl):
        if pl not in made:
            made[pl] = Torrent(tmp_path_factory.mktemp(f"t{pl}"), TORRENTS[pl], pl, seed=pl)
        return made[pl]

    return get


# ---- hashing: the leaf table ----------------------------------------------------

@pytest.mark.parametrize("pl", sorted(TORRENTS))
def test_hash_leaves_is_the_hashlib_table(pool, torrents, pl):
    from vortex_amd import merkle

    t = torrents(pl)
    rows, ok, tree, errs, leaves = pool.hash_merkle_files_leaves(t.paths, t.flens, pl)
    assert leaves == t.table == merkle.file_leaf_table(t.paths, t.flens, pl)
    assert rows == t.roots and ok == [True] * t.n and errs == 0
    assert (rows, ok, tree, errs) == pool.hash_merkle_files(t.paths, t.flens, pl)
    assert tree is not None
    # a range is a slice, and it has no tree
    for first, count in ((1, t.n - 2), (t.n - 1, 1), (0, 1)):
        r2, ok2, tree2, _, leaves2 = pool.hash_merkle_files_leaves(t.paths, t.flens, pl, first=first, count=count)
        lo, hi = t.first[first], t.first[first + count - 1] + t.blocks[first + count - 1]
        assert (r2, tree2, leaves2) == (rows[32 * first:32 * (first + count)], None, t.table[32 * lo:32 * hi])


def test_a_truncated_file_zeroes_the_rows_of_the_pieces_that_lack_bytes(pool, torrents, tmp_path):
    t = torrents(65536)
    paths = write_files(tmp_path, t.datas)
    os.truncate(paths[0], 65536 + 20000)  # pieces 1, 2, 3 of file 0 lack bytes; piece 0 does not
    os.unlink(paths[3])                    # pieces 7, 8
    rows, ok, tree, errs, leaves = pool.hash_merkle_files_leaves(paths, t.flens, 65536)
    lacking = {1, 2, 3, 7, 8}
    assert ok == [i not in lacking for i in range(t.n)] and errs == len(lacking)
    for i in range(t.n):
        want = bytes(32 * t.blocks[i]) if i in lacking else t.leaves(i)
        assert t.leaves(i, leaves) == want, i
        assert rows[32 * i:32 * i + 32] == (bytes(32) if i in lacking else t.roots[32 * i:32 * i + 32])


# ---- the closed loop ---------------------------------------------------------------

@pytest.mark.parametrize("pl", sorted(TORRENTS))
def test_closed_loop(pool, torrents, pl):
    t = torrents(pl)
    leaves = pool.hash_merkle_files_leaves(t.paths, t.flens, pl)[4]
    res = pool.verify_merkle_files_blocks(t.paths, t.flens, pl, t.roots, leaves)
    matched, layer_ok, bad, counts = res
    assert matched == [True] * t.n == pool.verify_merkle_files(t.paths, t.flens, pl, t.roots)[0]
    assert layer_ok == [True] * t.n and res.io_errors == 0
    assert bad == [0] * (t.n * t.wpp) and counts == [0] * t.n


# ---- damage ----------------------------------------------------------------------

def _expect(t, datas, table):
    """matched, layer_ok and the bad lists by hashlib."""
    from vortex_amd import merkle

    bad = {i: merkle.bad_blocks(t.piece(i, datas), t.leaves(i, table)) for i in range(t.n)}
    matched = [t.piece(i, datas) == t.piece(i) for i in range(t.n)]
    layer_ok = [t.root_of(t.leaves(i, table), t.log2w[i]) == t.roots[32 * i:32 * i + 32] for i in range(t.n)]
    return matched, layer_ok, bad


def _damaged(t, tmp_path, flips):
    """A copy of the torrent's files with one byte flipped at each (piece, byte of the piece)."""
    datas = [bytearray(d) for d in t.datas]
    paths = write_files(tmp_path, t.datas)
    for i, at in flips:
        datas[t.findex[i]][t.foff[i] + at] ^= 0x40
        flip(paths[t.findex[i]], t.foff[i] + at)
    return paths, [bytes(d) for d in datas]


def _corrupt_row(table, row):
    return table[:32 * row] + bytes([table[32 * row] ^ 1]) + table[32 * row + 1:]


def test_data_damage_names_the_blocks(pool, torrents, tmp_path):
    t = torrents(2 * MiB)
    flips = [(1, 5),                                    # the first block of a piece
             (0, 63 * BLOCK + 16383), (0, 64 * BLOCK),  # blocks 63 and 64 of a 2 MiB piece: two words
             (2, t.lens[2] - 1),                        # the short last block of the file
             (3, 100)]                                  # the one-block file
    paths, datas = _damaged(t, tmp_path, flips)
    matched, layer_ok, bad = _expect(t, datas, t.table)
    assert bad == {0: [63, 64], 1: [0], 2: [70], 3: [0], 4: [], 5: []}
    res = pool.verify_merkle_files_blocks(paths, t.flens, t.pl, t.roots, t.table)
    assert res.matched == matched == [False] * 4 + [True] * 2
    assert res.layer_ok == layer_ok == [True] * t.n
    assert res.bad == t.words(bad)
    assert res.bad_counts == [2, 1, 1, 1, 0, 0] and [res.blocks(i) for i in range(t.n)] == list(bad.values())
    assert res.matched == pool.verify_merkle_files(paths, t.flens, t.pl, t.roots)[0]


@pytest.mark.parametrize("pl", [16384, 65536, MiB])
def test_data_damage_at_every_piece_length(pool, torrents, tmp_path, pl):
    t = torrents(pl)
    flips = [(0, 0), (t.n - 1, t.lens[t.n - 1] - 1)] + [(i, t.lens[i] // 2) for i in range(2, t.n - 1, 3)]
    paths, datas = _damaged(t, tmp_path, flips)
    matched, layer_ok, bad = _expect(t, datas, t.table)
    res = pool.verify_merkle_files_blocks(paths, t.flens, pl, t.roots, t.table)
    assert (res.matched, res.layer_ok, res.bad) == (matched, layer_ok, t.words(bad))
    assert res.bad_counts == [len(bad[i]) for i in range(t.n)] and sum(res.bad_counts) == len(flips)
    assert layer_ok == [True] * t.n


def test_a_stale_stored_row_of_a_clean_piece(pool, torrents):
    t = torrents(2 * MiB)
    stale = _corrupt_row(t.table, t.first[1] + 64)  # piece 1, block 64
    res = pool.verify_merkle_files_blocks(t.paths, t.flens, t.pl, t.roots, stale)
    assert res.matched == [True] * t.n
    assert res.layer_ok == [i != 1 for i in range(t.n)]
    assert res.bad == t.words({1: [64]}) and res.bad_counts == [0, 1, 0, 0, 0, 0]
    matched, layer_ok, bad = _expect(t, t.datas, stale)
    assert (res.matched, res.layer_ok, res.bad) == (matched, layer_ok, t.words(bad))


def test_damaged_data_and_a_stale_row_in_one_piece(pool, torrents, tmp_path):
    t = torrents(MiB)
    paths, datas = _damaged(t, tmp_path, [(1, 3 * BLOCK + 1)])
    stale = _corrupt_row(t.table, t.first[1] + 40)
    matched, layer_ok, bad = _expect(t, datas, stale)
    assert bad[1] == [3, 40] and not matched[1] and not layer_ok[1]
    res = pool.verify_merkle_files_blocks(paths, t.flens, t.pl, t.roots, stale)
    assert (res.matched, res.layer_ok, res.bad) == (matched, layer_ok, t.words(bad))
    assert res.matched[1] is False and res.layer_ok[1] is False and res.bad_counts[1] == 2


def test_missing_and_short_files(pool, torrents, tmp_path):
    t = torrents(65536)
    paths = write_files(tmp_path, t.datas)
    os.truncate(paths[0], 65536 + 20000)  # pieces 1, 2, 3
    os.unlink(paths[3])                    # pieces 7, 8
    os.truncate(paths[5], BLOCK)           # piece 9: 3 blocks, one of them there
    lacking = [1, 2, 3, 7, 8, 9]
    before = pool.stats()
    plain, plain_errs = pool.verify_merkle_files(paths, t.flens, 65536, t.roots)
    mid = pool.stats()
    res = pool.verify_merkle_files_blocks(paths, t.flens, 65536, t.roots, t.table)
    after = pool.stats()
    assert res.matched == plain == [i not in lacking for i in range(t.n)]
    assert res.io_errors == plain_errs == len(lacking)
    for key in ("io_errors", "pieces_mismatched", "pieces_completed", "bytes_completed"):
        assert after[key] - mid[key] == mid[key] - before[key], key
    # every existing block of the pieces that lack bytes, and no other bit
    assert res.bad == t.words({i: list(range(t.blocks[i])) for i in lacking})
    assert res.bad_counts == [t.blocks[i] if i in lacking else 0 for i in range(t.n)]
    assert res.layer_ok == [True] * t.n  # it does not depend on the data


def test_a_piece_of_32_mib_a_tree_wider_than_a_node_tile(pool, tmp_path):
    pl = 32 * MiB
    t = Torrent(tmp_path, [pl], pl, seed=77)
    assert t.n == 1 and t.blocks == [2048] and t.wpp == 32
    rows, ok, _, _, leaves = pool.hash_merkle_files_leaves(t.paths, t.flens, pl)
    assert (rows, ok, leaves) == (t.roots, [True], t.table)
    for at in (0, 1000 * BLOCK + 5, pl - 1):
        flip(t.paths[0], at)
    res = pool.verify_merkle_files_blocks(t.paths, t.flens, pl, t.roots, t.table)
    assert (res.matched, res.layer_ok, res.bad_counts) == ([False], [True], [3])
    assert res.bad == t.words({0: [0, 1000, 2047]})
    stale = _corrupt_row(t.table, 513)
    res = pool.verify_merkle_files_blocks(t.paths, t.flens, pl, t.roots, stale)
    assert (res.matched, res.layer_ok) == ([False], [False]) and res.blocks(0) == [0, 513, 1000, 2047]


# ---- ranges, direct I/O, holes -------------------------------------------------------

def test_range_is_a_slice_and_direct_io_changes_nothing(built, gpu, torrents, tmp_path):
    from vortex_amd.hash_pool import HashPool

    t = torrents(MiB)
    paths, datas = _damaged(t, tmp_path, [(0, 5), (2, 0), (t.n - 1, 0)])
    stale = _corrupt_row(t.table, t.first[1] + 9)
    results = []
    for direct in (0, 1):
        with HashPool(16384, slots=2, slot_bytes=262144, direct_io=direct) as p:
            whole = p.verify_merkle_files_blocks(paths, t.flens, MiB, t.roots, stale)
            results.append(whole)
            for first, count in ((0, 0), (0, 1), (1, 2), (2, t.n - 2), (t.n - 1, 1), (1, t.n - 1)):
                r = p.verify_merkle_files_blocks(paths, t.flens, MiB, t.roots, stale, first=first, count=count)
                assert r.matched == whole.matched[first:first + count], (first, count)
                assert r.layer_ok == whole.layer_ok[first:first + count]
                assert r.bad == whole.bad[first * t.wpp:(first + count) * t.wpp]
                assert r.bad_counts == whole.bad_counts[first:first + count]
    assert results[0] == results[1]
    matched, layer_ok, bad = _expect(t, datas, stale)
    assert (results[0].matched, results[0].layer_ok, results[0].bad) == (matched, layer_ok, t.words(bad))


def test_skip_holes_gives_the_same_and_reads_less(built, gpu, tmp_path):
    from vortex_amd import merkle
    from vortex_amd.hash_pool import HashPool

    pl = MiB
    # piece 0 written but for blocks 8..39, piece 1 never written, piece 2 (short) written
    body = bytearray(2 * MiB + 5 * BLOCK + 77)
    body[:8 * BLOCK] = rand(1, 8 * BLOCK)
    body[40 * BLOCK:MiB] = rand(2, MiB - 40 * BLOCK)
    body[2 * MiB:] = rand(3, 5 * BLOCK + 77)
    body = bytes(body)
    path = make_file(tmp_path / "sparse", len(body),
                     [(0, body[:8 * BLOCK]), (40 * BLOCK, body[40 * BLOCK:MiB]), (2 * MiB, body[2 * MiB:])])
    flens = [len(body)]
    table = merkle.file_leaf_table([path], flens, pl)
    roots = b"".join(Torrent.root_of(table[32 * 64 * i:32 * 64 * (i + 1)], 6) for i in range(3))
    stale = _corrupt_row(_corrupt_row(table, 20), 64 + 7)  # rows over holes: piece 0 block 20, piece 1 block 7
    got = {}
    with HashPool(16384, slots=3, slot_bytes=262144) as p:
        for skip in (False, True):
            p.skip_holes = skip
            clean = p.verify_merkle_files_blocks([path], flens, pl, roots, table)
            read = p.last_verify()["read_bytes"]
            trace = p.last_verify_holes()
            hit = p.verify_merkle_files_blocks([path], flens, pl, roots, stale)
            got[skip] = (clean, hit, read, trace)
    for skip in (False, True):
        clean, hit = got[skip][:2]
        assert (clean.matched, clean.layer_ok, clean.bad_counts) == ([True] * 3, [True] * 3, [0] * 3)
        assert (hit.matched, hit.layer_ok) == ([True] * 3, [False, False, True])
        assert [hit.blocks(i) for i in range(3)] == [[20], [7], []]
    assert got[True][:2] == got[False][:2]
    assert got[False][3]["hole_blocks"] == 0 and got[False][2] == len(body)
    if holes_reported(tmp_path):  # (else: NO_HOLES, and the verdicts above are all there is to check)
        assert got[True][3]["hole_blocks"] > 0 and got[True][2] < len(body), NO_HOLES


# ---- argument errors ------------------------------------------------------------------

def test_argument_errors_launch_nothing(pool, torrents):
    from vortex_amd._lib import VX_EBUSY, VX_EINVAL, VxError

    t = torrents(65536)
    before = pool.stats()
    for leaves in (t.table + bytes(32), t.table[:-32]):  # leaf_rows wrong
        with pytest.raises(VxError) as e:
            pool.verify_merkle_files_blocks(t.paths, t.flens, 65536, t.roots, leaves)
        assert e.value.code == VX_EINVAL and "leaf_rows" in str(e.value)
    arr = (ctypes.c_char_p * len(t.paths))(*[os.fsencode(p) for p in t.paths])
    lens = (ctypes.c_uint64 * len(t.flens))(*t.flens)
    out = ctypes.create_string_buffer(t.n)
    leaf_buf = ctypes.create_string_buffer(t.table, len(t.table))
    L = pool.lib
    rows_buf = ctypes.create_string_buffer(32 * t.n)
    assert L.vx_merkle_hash_files_leaves(pool._h, arr, lens, len(t.paths), 65536, t.n, rows_buf, None, None, 0,
                                         leaf_buf, t.rows + 1, 0) == VX_EINVAL
    assert L.vx_merkle_verify_files_blocks(pool._h, arr, lens, len(t.paths), 65536, t.roots, t.n, leaf_buf, t.rows, out,
                                           None, None, None, 0) == VX_EINVAL  # NULL bad_out
    assert b"NULL" in L.vx_last_error()
    assert pool.stats() == before
    body = rand(9, 16384)
    pool.spawn(0, 1, bytearray(body), len(body), hashlib.sha1(body).digest())
    for call in (lambda: pool.verify_merkle_files_blocks(t.paths, t.flens, 65536, t.roots, t.table),
                 lambda: pool.hash_merkle_files_leaves(t.paths, t.flens, 65536)):
        with pytest.raises(VxError) as e:
            call()
        assert e.value.code == VX_EBUSY
    pool.drain()
    assert pool.try_recv().hash_matched
    res = pool.verify_merkle_files_blocks(t.paths, t.flens, 65536, t.roots, t.table)  # the pool works on
    assert res.matched == [True] * t.n and res.bad_counts == [0] * t.n
