"""GPU: hashing files into torrent metadata — vx_hash_files (v1 `pieces`),
vx_merkle_hash_files (v2 rows and layer trees) and vx_hybrid_hash_files (both in
one pass), their _range forms, and the loop closed through the verify call of
each kind.

The yardsticks are hashlib over the files' bytes and the Python models
(merkle.build_tree, merkle.layer_root, hybrid.v1_digest, hybrid.v2_root); the
references of a layout are computed once per module.  Data is
np.random.default_rng(seed) bytes in a temporary directory.
"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
LENS = [200000, 1, 65537, 100000, 0, 49152]
# name -> (file lengths, piece length)
LAYOUTS = {
    "mixed-16k": (LENS, 16384),
    "mixed-64k": (LENS, 65536),
    "mixed-1m": (LENS, 1 << 20),
    "two-pass-tree": ([513 * BLOCK - 5], 16384),           # 513 rows: a tree of two passes; the last piece is short
    "wide-pieces": ([(16 << 20) + 1, 600 * BLOCK - 3], 16 << 20),  # piece trees wider than a node tile
}


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Torrent:
    """The files of one layout on disk and every table a hash call must return for them."""

    def __init__(self, root, name):
        from vortex_amd import hybrid, merkle

        self.flens, self.pl = LAYOUTS[name]
        self.datas = [random_bytes(1000 + 7 * k + len(name), n) for k, n in enumerate(self.flens)]
        os.makedirs(root, exist_ok=True)
        self.paths = []
        for k, d in enumerate(self.datas):
            self.paths.append(os.path.join(str(root), f"f{k:02d}.bin"))
            with open(self.paths[-1], "wb") as f:
                f.write(d)
        pl = self.pl
        # v1: pieces run across the files
        whole = b"".join(self.datas)
        self.v1 = [hashlib.sha1(whole[o:o + pl]).digest() for o in range(0, len(whole), pl)]
        # v2 and hybrid: every file starts its own pieces
        self.findex, self.foff, dlen, self.pads, lw = hybrid.hybrid_pieces(self.flens, pl)
        parts = [self.datas[f][o:o + n] for f, o, n in zip(self.findex, self.foff, dlen)]
        self.rows = [hybrid.v2_root(p, w) for p, w in zip(parts, lw)]
        self.hybrid_v1 = [hybrid.v1_digest(p, pad) for p, pad in zip(parts, self.pads)]
        height = merkle.log2_width(pl)
        self.counts, self.tree_off = merkle.tree_layout(self.flens, pl)
        self.trees, self.roots = [], []
        at = 0
        for c in self.counts:
            rows = self.rows[at:at + c]
            at += c
            self.trees.append(merkle.build_tree(rows, height) if c else b"")
            self.roots.append(merkle.layer_root(rows, height) if c else None)
        assert at == len(self.rows)

    def file_trees(self, tree):
        return [tree[32 * a:32 * b] for a, b in zip(self.tree_off, self.tree_off[1:])]


@pytest.fixture(scope="module")
def torrents(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Torrent(tmp_path_factory.mktemp(name), name)
        return made[name]

    return get


@pytest.fixture(scope="module")
def pool(built, gpu):
    """Three 4 MiB slots: the larger layouts take several rounds."""
    from vortex_amd.hash_pool import HashPool

    p = HashPool(16384, slots=3, slot_bytes=4 << 20)
    yield p
    p.close()


def _flip(path, at):
    with open(path, "r+b") as f:
        f.seek(at)
        b = f.read(1)
        f.seek(at)
        f.write(bytes([b[0] ^ 1]))


# ---- v1 --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed-16k", "mixed-64k"])
def test_v1_pieces_span_files(pool, torrents, name):
    t = torrents(name)
    st0 = pool.stats()
    dig, ok, bad = pool.hash_files(t.paths, t.flens, t.pl, io_threads=3)
    assert dig == b"".join(t.v1) and ok == [True] * len(t.v1) and bad == 0
    st1 = pool.stats()
    assert st1["pieces_completed"] - st0["pieces_completed"] == len(t.v1)
    assert st1["bytes_completed"] - st0["bytes_completed"] == sum(t.flens)
    assert st1["pieces_mismatched"] == st0["pieces_mismatched"] and st1["io_errors"] == st0["io_errors"]
    lv = pool.last_verify()
    assert lv["read_bytes"] == sum(t.flens) and lv["readers"] == 3
    # the loop closed: the table verifies the files it was made from
    assert pool.verify_files(t.paths, t.flens, t.pl, dig) == ([True] * len(t.v1), 0)
    # a slice is a slice of the whole
    n = len(t.v1)
    sub, sub_ok, sub_bad = pool.hash_files(t.paths, t.flens, t.pl, first=2, count=n - 3)
    assert (sub, sub_ok, sub_bad) == (dig[40:20 * (n - 1)], [True] * (n - 3), 0)


def test_v1_a_piece_over_several_chunk_rounds(built, gpu, tmp_path):
    """A context whose chunk is 12,288 bytes: a 300,000-byte piece takes 25
    rounds and the state crosses every one of them."""
    from vortex_amd.hash_pool import HashPool

    pl, chunk = 300000, 12288
    sizes = [3 * pl + 777, 0, 5 * pl + 64, pl // 3]
    paths = []
    for k, n in enumerate(sizes):
        p = tmp_path / f"s{k}.bin"
        p.write_bytes(random_bytes(40 + k, n))
        paths.append(str(p))
    data = b"".join(open(p, "rb").read() for p in paths)
    want = b"".join(hashlib.sha1(data[i:i + pl]).digest() for i in range(0, len(data), pl))
    with HashPool(pl, slots=3, batch_pieces=4, slot_bytes=4 << 20, verify_chunk=chunk, verify_ramp=1) as p:
        r0 = p.stats()["chunk_rounds"]
        dig, ok, bad = p.hash_files(paths, sizes, pl, io_threads=3)
        rounds = p.stats()["chunk_rounds"] - r0
        assert dig == want and all(ok) and bad == 0
        assert rounds >= (pl + chunk - 1) // chunk
        _flip(paths[2], 2 * pl - 100)
        assert p.verify_files(paths, sizes, pl, dig)[0].count(False) == 1


# ---- v2 --------------------------------------------------------------------------

def _check_v2(t, rows, ok, tree, bad):
    from vortex_amd import merkle

    assert rows == b"".join(t.rows) and ok == [True] * len(t.rows) and bad == 0
    assert len(tree) == 32 * t.tree_off[-1]
    got = t.file_trees(tree)
    for f, (g, w) in enumerate(zip(got, t.trees)):
        assert g == w, f"tree of file {f} ({t.flens[f]} bytes)"
        if w:
            assert g[-32:] == t.roots[f]  # the file's `pieces root`
            assert g[:32 * t.counts[f]] == b"".join(t.rows)[32 * sum(t.counts[:f]):32 * sum(t.counts[:f + 1])]
    assert merkle.tree_layout(t.flens, t.pl) == (t.counts, t.tree_off)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_v2_rows_and_trees(pool, torrents, name):
    t = torrents(name)
    st0 = pool.stats()
    rows, ok, tree, bad = pool.hash_merkle_files(t.paths, t.flens, t.pl)
    _check_v2(t, rows, ok, tree, bad)
    st1 = pool.stats()
    assert st1["pieces_completed"] - st0["pieces_completed"] == len(t.rows)
    assert st1["bytes_completed"] - st0["bytes_completed"] == sum(t.flens)
    assert st1["batches"] > st0["batches"] and st1["pieces_mismatched"] == st0["pieces_mismatched"]
    assert pool.last_verify()["read_bytes"] == sum(t.flens)
    assert pool.verify_merkle_files(t.paths, t.flens, t.pl, rows) == ([True] * len(t.rows), 0)
    if name == "two-pass-tree":
        assert t.counts == [513] and len(tree) == 32 * 1034
    no_tree = pool.hash_merkle_files(t.paths, t.flens, t.pl, trees=False)
    assert no_tree == (rows, ok, None, 0)


@pytest.mark.parametrize("name", ["mixed-64k", "two-pass-tree"])
def test_v2_range_is_a_slice(pool, torrents, name):
    t = torrents(name)
    n = len(t.rows)
    rows, ok, tree, bad = pool.hash_merkle_files(t.paths, t.flens, t.pl, first=1, count=n - 2)
    assert (rows, ok, tree, bad) == (b"".join(t.rows[1:n - 1]), [True] * (n - 2), None, 0)
    assert pool.last_verify()["read_bytes"] < sum(t.flens)


# ---- hybrid ----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_hybrid_both_tables_in_one_pass(pool, torrents, name):
    t = torrents(name)
    st0 = pool.stats()
    sha1, rows, ok, tree, bad = pool.hash_hybrid_files(t.paths, t.flens, t.pl)
    assert sha1 == b"".join(t.hybrid_v1)
    _check_v2(t, rows, ok, tree, bad)
    st1 = pool.stats()
    assert st1["pieces_completed"] - st0["pieces_completed"] == len(t.rows)
    assert st1["bytes_completed"] - st0["bytes_completed"] == sum(t.flens)
    assert st1["pieces_mismatched"] == st0["pieces_mismatched"]
    assert pool.last_verify()["read_bytes"] == sum(t.flens)  # the pads are hashed but never read
    assert pool.verify_hybrid_files(t.paths, t.flens, t.pl, sha1, rows) == [(True, True)] * len(t.rows)
    n = len(t.rows)
    if n > 2:
        sub = pool.hash_hybrid_files(t.paths, t.flens, t.pl, first=1, count=n - 2)
        assert sub == (sha1[20:20 * (n - 1)], rows[32:32 * (n - 1)], [True] * (n - 2), None, 0)


# ---- the loop closed: a flipped byte fails exactly its piece ----------------------

def test_flipped_byte_fails_exactly_its_piece(pool, tmp_path):
    t = Torrent(tmp_path, "mixed-64k")
    v1, _, _ = pool.hash_files(t.paths, t.flens, t.pl)
    rows, _, _, _ = pool.hash_merkle_files(t.paths, t.flens, t.pl)
    hv1, hrows, _, _, _ = pool.hash_hybrid_files(t.paths, t.flens, t.pl)
    # byte 70,000 of file 3: v2 piece 7 + 1 = 8 (files 0-2 hold 4 + 1 + 2 pieces); v1 byte 200000 + 1 + 65537 + 70000
    _flip(t.paths[3], 70000)
    v1_piece = (200000 + 1 + 65537 + 70000) // t.pl
    assert pool.verify_files(t.paths, t.flens, t.pl, v1)[0] == [i != v1_piece for i in range(len(t.v1))]
    assert pool.verify_merkle_files(t.paths, t.flens, t.pl, rows)[0] == [i != 8 for i in range(len(t.rows))]
    assert pool.verify_hybrid_files(t.paths, t.flens, t.pl, hv1, hrows) == \
        [(i != 8, i != 8) for i in range(len(t.rows))]
    # and hashing again gives new rows for exactly that piece, a new tree for exactly that file
    rows2, _, tree2, _ = pool.hash_merkle_files(t.paths, t.flens, t.pl)
    assert [i for i in range(len(t.rows)) if rows2[32 * i:32 * i + 32] != t.rows[i]] == [8]
    assert [f for f, (g, w) in enumerate(zip(t.file_trees(tree2), t.trees)) if g != w] == [3]


# ---- faults ----------------------------------------------------------------------

def test_missing_and_truncated_files(pool, tmp_path):
    """File 2 is gone and file 0 is cut to 150,000 bytes: ok == 0 and zero rows
    for exactly the pieces that lack bytes, a zero tree for those two files
    only, and the return value counts the pieces."""
    t = Torrent(tmp_path, "mixed-64k")
    os.remove(t.paths[2])
    with open(t.paths[0], "r+b") as f:
        f.truncate(150000)
    pl = t.pl
    # v2 numbering: file 0 is pieces 0-3 (2 and 3 lie past byte 150,000, piece 2 in part), file 2 pieces 5-6
    lacking = {2, 3, 5, 6}
    n = len(t.rows)
    want_ok = [i not in lacking for i in range(n)]
    want_rows = b"".join(bytes(32) if i in lacking else t.rows[i] for i in range(n))
    want_trees = [bytes(len(w)) if f in (0, 2) else w for f, w in enumerate(t.trees)]
    io0 = pool.stats()["io_errors"]
    rows, ok, tree, bad = pool.hash_merkle_files(t.paths, t.flens, pl)
    assert (rows, ok, bad) == (want_rows, want_ok, 4)
    assert t.file_trees(tree) == want_trees
    assert pool.stats()["io_errors"] - io0 == 4
    sha1, rows, ok, tree, bad = pool.hash_hybrid_files(t.paths, t.flens, pl)
    assert (rows, ok, bad) == (want_rows, want_ok, 4)
    assert sha1 == b"".join(bytes(20) if i in lacking else t.hybrid_v1[i] for i in range(n))
    assert t.file_trees(tree) == want_trees
    # v1: a piece lacks bytes where its range meets [150000, 200000) or file 2's [200001, 265538)
    holes = [(150000, 200000), (200001, 200001 + 65537)]
    v1_lacking = {i for i in range(len(t.v1)) if any(lo < (i + 1) * pl and i * pl < hi for lo, hi in holes)}
    dig, ok, bad = pool.hash_files(t.paths, t.flens, pl)
    assert ok == [i not in v1_lacking for i in range(len(t.v1))] and bad == len(v1_lacking) > 0
    assert dig == b"".join(bytes(20) if i in v1_lacking else t.v1[i] for i in range(len(t.v1)))


# ---- options -----------------------------------------------------------------------

def test_io_threads_and_direct_io_change_no_byte(built, gpu, torrents):
    from vortex_amd.hash_pool import HashPool

    t = torrents("mixed-1m")
    for direct in (0, 1):
        with HashPool(16384, slots=3, slot_bytes=4 << 20, direct_io=direct) as p:
            for threads in (1, 4):
                assert p.hash_files(t.paths, t.flens, t.pl, io_threads=threads)[0] == b"".join(t.v1)
                rows, ok, tree, bad = p.hash_merkle_files(t.paths, t.flens, t.pl, io_threads=threads)
                _check_v2(t, rows, ok, tree, bad)
                assert p.last_verify()["readers"] == threads
                sha1, rows, ok, tree, bad = p.hash_hybrid_files(t.paths, t.flens, t.pl, io_threads=threads)
                assert sha1 == b"".join(t.hybrid_v1)
                _check_v2(t, rows, ok, tree, bad)


def test_busy_while_async_pieces_are_pending(pool, torrents):
    from vortex_amd._lib import VX_EBUSY, VxError

    t = torrents("mixed-16k")
    body = random_bytes(9, 16384)
    pool.spawn(0, 1, bytearray(body), len(body), hashlib.sha1(body).digest())
    for call in (pool.hash_files, pool.hash_merkle_files, pool.hash_hybrid_files):
        with pytest.raises(VxError) as e:
            call(t.paths, t.flens, t.pl)
        assert e.value.code == VX_EBUSY
    pool.drain()
    assert pool.try_recv().hash_matched
    assert pool.hash_files(t.paths, t.flens, t.pl)[0] == b"".join(t.v1)
