"""GPU: the BitTorrent v2 re-verify from disk — the block-stream leaf kernel
behind vx_merkle_device_blocks, vx_merkle_device_nodes, and
vx_merkle_verify_files / _range.

The yardstick is hashlib.sha256 and the pure-Python BEP 52 tree below.
Everything is bit-exact.  Data is np.random.default_rng(seed) bytes in
tmp_path; no case needs more than a few MB.
"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
EDGES = [0, 1, 55, 56, 63, 64, 127, 128, 16383, 16384]  # the SHA-256 padding edges


def sha256(b):
    return hashlib.sha256(b).digest()


def piece_root(data, log2w):
    """BEP 52: leaves over 16 KiB blocks (the last at its real length), zero
    hashes beyond the data, a binary tree over 2^log2w leaf slots."""
    nodes = [sha256(data[o:o + BLOCK]) if o < len(data) else bytes(32) for o in range(0, BLOCK << log2w, BLOCK)]
    while len(nodes) > 1:
        nodes = [sha256(nodes[k] + nodes[k + 1]) for k in range(0, len(nodes), 2)]
    return nodes[0]


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def torrent_roots(datas, pl):
    """The `expected` table of a torrent from its files' bytes: every file's
    pieces in order, full width for a file longer than pl, else the file's own."""
    full = (pl // BLOCK).bit_length() - 1
    out = []
    for d in datas:
        if len(d) > pl:
            out += [piece_root(d[o:o + pl], full) for o in range(0, len(d), pl)]
        elif d:
            out.append(piece_root(d, (-(-len(d) // BLOCK) - 1).bit_length()))
    return out


def write_files(root, datas):
    os.makedirs(root, exist_ok=True)
    paths = []
    for k, d in enumerate(datas):
        p = os.path.join(str(root), f"f{k:04d}.bin")
        with open(p, "wb") as f:
            f.write(d)
        paths.append(p)
    return paths


# ---- device entries ----------------------------------------------------------

def test_blocks_any_mix_against_hashlib(built, gpu):
    """300 blocks (two workgroups, not a multiple of 64), lengths mixed from the
    padding edges, rows permuted, some skipped; the stage is 0xFF wherever a
    block has no bytes and is followed by a 0xFF guard, the leaves are 0xFF
    before the call; five more absent entries lie past the end of the stage."""
    import torch

    from vortex_amd import device as vdev

    rng = np.random.default_rng(11)
    n, extra, rows_total = 300, 5, 330
    lens = [EDGES[k % len(EDGES)] for k in range(n)]
    rng.shuffle(lens)
    lens[-1] = 55  # the last block of the stage is short: nothing after it may matter
    lens += [0] * extra
    perm = rng.permutation(rows_total)[:n + extra].tolist()
    skipped = set(range(7, n, 13)) | {n + 1}
    rows = [vdev.SKIP_ROW if b in skipped else perm[b] for b in range(n + extra)]
    stage = bytearray(b"\xff" * (n * BLOCK + BLOCK))  # (+ the guard)
    blocks = []
    for b in range(n):
        d = random_bytes(1000 + b, lens[b])
        stage[b * BLOCK:b * BLOCK + lens[b]] = d
        blocks.append(d)
    blocks += [b""] * extra
    want = bytearray(b"\xff" * (32 * rows_total))
    for b in range(n + extra):
        if b not in skipped:
            want[32 * rows[b]:32 * rows[b] + 32] = sha256(blocks[b]) if lens[b] else bytes(32)

    d_stage = torch.frombuffer(stage, dtype=torch.uint8).to(gpu)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for dtype in (torch.int64, torch.int32):
        vals = rows if dtype == torch.int64 else [r if r < 1 << 31 else r - (1 << 32) for r in rows]
        d_rows = torch.tensor(vals, dtype=dtype, device=gpu)
        leaves = torch.full((rows_total, 32), 0xFF, dtype=torch.uint8, device=gpu)
        vdev.merkle_blocks(d_stage, d_rows, d_lens, leaves)
        torch.cuda.synchronize()
        got = leaves.cpu().numpy().tobytes()
        bad = [k for k in range(rows_total) if got[32 * k:32 * k + 32] != bytes(want[32 * k:32 * k + 32])]
        assert not bad, f"{len(bad)} leaf rows differ, first {bad[0]}"
    # the on-device argument checks
    leaves = torch.full((rows_total, 32), 0xFF, dtype=torch.uint8, device=gpu)
    d_rows = torch.tensor(rows, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError, match="outside leaves"):
        over = torch.tensor(rows[:-1] + [rows_total], dtype=torch.int64, device=gpu)
        vdev.merkle_blocks(d_stage, over, d_lens, leaves)
    with pytest.raises(ValueError, match="0..16384"):
        vdev.merkle_blocks(d_stage, d_rows, torch.tensor(lens[:-1] + [16385], dtype=torch.int32, device=gpu), leaves)
    with pytest.raises(ValueError, match="past the stage"):
        vdev.merkle_blocks(d_stage, d_rows, torch.tensor(lens[:-1] + [1], dtype=torch.int32, device=gpu), leaves)
    with pytest.raises(ValueError, match="differ in length"):
        vdev.merkle_blocks(d_stage, d_rows[:-1], d_lens, leaves)
    torch.cuda.synchronize()
    assert leaves.cpu().numpy().tobytes() == b"\xff" * (32 * rows_total)  # a refused call wrote nothing
    vdev.merkle_blocks(d_stage, d_rows[:0], d_lens[:0], leaves)  # n == 0 launches nothing


def test_blocks_then_nodes_equals_ragged(built, gpu):
    """75 pieces of 4 leaf slots (300 blocks): blocks + nodes gives exactly
    what merkle_ragged gives for the same bytes, and what the Python tree says."""
    import torch

    from vortex_amd import device as vdev

    n, lw_full = 75, 2
    tails = [e for e in EDGES if e]
    pieces, log2w = [], []
    for i in range(n):
        nb = 1 + i % 4
        tail = tails[(i * 5 + 2) % len(tails)]
        pieces.append(random_bytes(2000 + i, (nb - 1) * BLOCK + tail))
        log2w.append((nb - 1).bit_length() if i % 3 else lw_full)  # a file's own width, or the full one
    stage = bytearray(b"\xff" * (n * 4 * BLOCK + BLOCK))
    rows, lens = [], []
    for i, p in enumerate(pieces):
        stage[i * 4 * BLOCK:i * 4 * BLOCK + len(p)] = p
        for k in range(4):
            rows.append(4 * i + k)
            lens.append(max(0, min(BLOCK, len(p) - k * BLOCK)))
    roots_want = [piece_root(p, w) for p, w in zip(pieces, log2w)]
    expected = list(roots_want)
    expected[9] = bytes(32)
    expected[40] = roots_want[41]

    d_stage = torch.frombuffer(stage, dtype=torch.uint8).to(gpu)
    d_lw = torch.tensor(log2w, dtype=torch.uint8, device=gpu)
    d_exp = torch.frombuffer(bytearray(b"".join(expected)), dtype=torch.uint8).to(gpu)
    r_roots, r_leaves, r_m = vdev.merkle_ragged(
        d_stage, torch.tensor([i * 4 * BLOCK for i in range(n)], dtype=torch.int64, device=gpu),
        torch.tensor([len(p) for p in pieces], dtype=torch.int32, device=gpu), lw_full, log2w=d_lw, expected=d_exp,
        leaves=torch.full((n * 4, 32), 0xFF, dtype=torch.uint8, device=gpu))
    # the blocks in a shuffled order: a lane's position says nothing about its row
    order = np.random.default_rng(5).permutation(4 * n).tolist()
    sh_stage = bytearray(len(stage))
    for b, src in enumerate(order):
        sh_stage[b * BLOCK:(b + 1) * BLOCK] = stage[src * BLOCK:(src + 1) * BLOCK]
    sh_stage[4 * n * BLOCK:] = b"\xff" * BLOCK
    leaves = torch.full((n * 4, 32), 0xFF, dtype=torch.uint8, device=gpu)
    vdev.merkle_blocks(torch.frombuffer(sh_stage, dtype=torch.uint8).to(gpu),
                       torch.tensor([rows[s] for s in order], dtype=torch.int64, device=gpu),
                       torch.tensor([lens[s] for s in order], dtype=torch.int32, device=gpu), leaves)
    b_roots, b_m = vdev.merkle_nodes(leaves, n, lw_full, log2w=d_lw, expected=d_exp)
    torch.cuda.synchronize()
    assert leaves.cpu().numpy().tobytes() == r_leaves.cpu().numpy().tobytes()
    got = b_roots.cpu().numpy().tobytes()
    assert got == r_roots.cpu().numpy().tobytes() == b"".join(roots_want)
    want_m = [int(i not in (9, 40)) for i in range(n)]
    assert b_m.cpu().tolist() == r_m.cpu().tolist() == want_m
    # without log2w every tree is full width; roots only
    f_roots, f_m = vdev.merkle_nodes(leaves, n, lw_full)
    torch.cuda.synchronize()
    assert f_m is None and f_roots.cpu().numpy().tobytes() == b"".join(piece_root(p, lw_full) for p in pieces)


# ---- files ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool(built, gpu):
    """Three 4 MiB slots: every torrent below takes several rounds."""
    from vortex_amd.hash_pool import HashPool

    p = HashPool(16384, slots=3, slot_bytes=4 << 20)
    yield p
    p.close()


_TORRENTS = {}


@pytest.fixture(scope="module")
def torrent(tmp_path_factory):
    """The issue's torrent at a piece length, built once: (paths, file lengths,
    expected rows, file bytes)."""
    def make(pl):
        if pl not in _TORRENTS:
            rng = np.random.default_rng(pl)
            flens = [0, 1, 16384, 16385, 3 * BLOCK, pl, pl + 1, 2 * pl + 5] + rng.integers(1, 40001, 300).tolist()
            datas = [random_bytes(31 * pl + k, n) for k, n in enumerate(flens)]
            paths = write_files(tmp_path_factory.mktemp(f"t{pl}"), datas)
            _TORRENTS[pl] = (paths, flens, torrent_roots(datas, pl), datas)
        return _TORRENTS[pl]
    return make


@pytest.mark.parametrize("pl", [16384, 65536, 1 << 20])
def test_files_against_python_tree(pool, torrent, pl):
    from vortex_amd import merkle

    paths, flens, roots, _ = torrent(pl)
    lens, log2w, findex, _ = merkle.torrent_pieces(flens, pl)
    n = len(roots)
    assert n == len(lens) > 256  # more pieces than a node workgroup has threads
    got, bad = pool.verify_merkle_files(paths, flens, pl, b"".join(roots))
    assert bad == 0
    assert got == [True] * n, [i for i, ok in enumerate(got) if not ok][:10]
    # a wrong expected row fails that piece and no other
    wrong = list(roots)
    for i in (0, 5, n // 2, n - 1):
        wrong[i] = sha256(roots[i])
    got, bad = pool.verify_merkle_files(paths, flens, pl, b"".join(wrong))
    assert bad == 0 and [i for i, ok in enumerate(got) if not ok] == sorted({0, 5, n // 2, n - 1})
    # a root at the wrong width is a wrong root: the single piece of the 3-block file at full width
    if pl > 65536:
        i = findex.index(4)
        assert log2w[i] == 2
        wrong = list(roots)
        wrong[i] = piece_root(open(paths[4], "rb").read(), (pl // BLOCK).bit_length() - 1)
        got, _ = pool.verify_merkle_files(paths, flens, pl, b"".join(wrong))
        assert [k for k, ok in enumerate(got) if not ok] == [i]


def test_piece_larger_than_a_round_and_than_max_piece_len(built, gpu, tmp_path):
    """1 MiB pieces through 256 KiB slots of a 16 KiB pool: the piece length is
    bounded by neither; the host batch on a pool large enough agrees."""
    from vortex_amd.hash_pool import HashPool

    pl = 1 << 20
    data = random_bytes(77, 5 * pl // 2 + 5)
    paths = write_files(tmp_path, [data])
    roots = torrent_roots([data], pl)
    assert len(roots) == 3
    with HashPool(16384, slots=2, slot_bytes=262144) as small:
        small.reset_stats()
        got, bad = small.verify_merkle_files(paths, [len(data)], pl, b"".join(roots), io_threads=3)
        assert (got, bad) == ([True] * 3, 0)
        st, lv = small.stats(), small.last_verify()
        assert st["pieces_completed"] == 3 and st["pieces_mismatched"] == 0 and st["io_errors"] == 0
        assert st["bytes_completed"] == len(data)
        rounds = -(-len(data) // 262144)
        assert st["batches"] == lv["rounds"] == rounds > 1
        assert lv["chunk_bytes"] == 262144 and lv["readers"] == 3 and lv["wall_ms"] > 0
        assert lv["read_bytes"] == len(data) and lv["copy_bytes"] == len(data)
        assert lv["tail_ms"] >= 0 and lv["read_busy_ms"] > 0
        assert small.last_verify_rounds() == []
        wrong = [roots[0], sha256(roots[1]), roots[2]]
        got, bad = small.verify_merkle_files(paths, [len(data)], pl, b"".join(wrong))
        assert (got, bad) == ([True, False, True], 0)
        assert small.stats()["pieces_mismatched"] == 1
    with HashPool(pl) as big:
        pieces = [data[o:o + pl] for o in range(0, len(data), pl)]
        verdicts, batch_roots = big.verify_merkle(pieces, roots, pl)
        assert verdicts == [True] * 3 and batch_roots == roots
        got, bad = big.verify_merkle_files(paths, [len(data)], pl, b"".join(roots))
        assert (got, bad) == ([True] * 3, 0)


def test_tree_wider_than_a_node_tile(pool, tmp_path):
    """16 MiB pieces are trees of 1,024 leaves, reduced by the wide node kernel
    (one workgroup per piece, tile by tile): a file of 16 MiB + 1 byte is one
    full piece over five rounds and one piece of a 1-byte block and 1,023
    absent slots; a 600-block file beside it is a single piece of its own
    width 1,024."""
    pl = 16 << 20
    datas = [random_bytes(91, pl + 1), random_bytes(92, 600 * BLOCK - 3)]
    paths = write_files(tmp_path, datas)
    roots = torrent_roots(datas, pl)
    assert len(roots) == 3
    flens = [len(d) for d in datas]
    got, bad = pool.verify_merkle_files(paths, flens, pl, b"".join(roots))
    assert (got, bad) == ([True] * 3, 0)
    for i in range(3):
        wrong = list(roots)
        wrong[i] = sha256(roots[i])
        got, bad = pool.verify_merkle_files(paths, flens, pl, b"".join(wrong))
        assert (got, bad) == ([k != i for k in range(3)], 0)
    with open(paths[0], "r+b") as f:  # one byte in the last tile of the first piece
        f.seek(pl - 5)
        f.write(bytes([datas[0][pl - 5] ^ 1]))
    got, bad = pool.verify_merkle_files(paths, flens, pl, b"".join(roots))
    assert (got, bad) == ([False, True, True], 0)


DAMAGE_PL = 65536
DAMAGE_LENS = [200000, 1, 65537, 100000, 0, 3 * BLOCK]  # pieces 0-3 | 4 | 5-6 | 7-8 | - | 9


@pytest.fixture(scope="module")
def damage_torrent():
    datas = [random_bytes(500 + k, n) for k, n in enumerate(DAMAGE_LENS)]
    return datas, torrent_roots(datas, DAMAGE_PL)


def _flip(path, at):
    with open(path, "r+b") as f:
        f.seek(at)
        b = f.read(1)
        f.seek(at)
        f.write(bytes([b[0] ^ 0x40]))


@pytest.mark.parametrize("case,fails,io_errors", [
    ("flip_middle_block", (1,), 0),      # a byte of the third block of piece 1
    ("flip_last_short_block", (3,), 0),  # the file's last byte
    ("truncate_mid_piece", (1, 2, 3), 3),
    ("missing_file", (5, 6), 2),
    ("truncate_to_block_boundary", (7, 8), 2),  # file 3 cut to 16 KiB: piece 7 lacks bytes too
    ("longer_than_declared", (), 0),
])
def test_damage(pool, damage_torrent, tmp_path, case, fails, io_errors):
    datas, roots = damage_torrent
    paths = write_files(tmp_path, datas)
    if case == "flip_middle_block":
        _flip(paths[0], DAMAGE_PL + 2 * BLOCK + 77)
    elif case == "flip_last_short_block":
        _flip(paths[0], DAMAGE_LENS[0] - 1)
    elif case == "truncate_mid_piece":
        os.truncate(paths[0], DAMAGE_PL + 20000)
    elif case == "missing_file":
        os.unlink(paths[2])
    elif case == "truncate_to_block_boundary":
        os.truncate(paths[3], BLOCK)
    else:
        with open(paths[1], "ab") as f:
            f.write(b"more than the torrent says")
    before = pool.stats()
    got, bad = pool.verify_merkle_files(paths, DAMAGE_LENS, DAMAGE_PL, b"".join(roots))
    assert tuple(i for i, ok in enumerate(got) if not ok) == fails and len(got) == len(roots) == 10
    assert bad == io_errors
    after = pool.stats()
    assert after["io_errors"] - before["io_errors"] == io_errors
    assert after["pieces_mismatched"] - before["pieces_mismatched"] == len(fails) - io_errors
    assert after["pieces_completed"] - before["pieces_completed"] == 10


def test_range_is_a_slice_of_the_whole(pool, torrent):
    pl = 65536
    paths, flens, roots, _ = torrent(pl)
    n = len(roots)
    wrong = list(roots)
    for i in (2, 7, 9, 100, n - 1):
        wrong[i] = bytes(32)
    exp = b"".join(wrong)
    whole, _ = pool.verify_merkle_files(paths, flens, pl, exp)
    assert whole.count(False) == 5
    # pieces 0-3 are the first four files', 4 | 5-6 | 7-9 the next three's: ranges that cut files
    for first, count in ((0, 0), (0, 1), (1, 5), (6, 1), (6, 2), (5, 4), (8, 120), (n - 3, 3), (n, 0), (3, n - 3)):
        pool.reset_stats()
        got, bad = pool.verify_merkle_files(paths, flens, pl, exp, first=first, count=count)
        assert (got, bad) == (whole[first:first + count], 0), (first, count)
        assert pool.stats()["pieces_completed"] == count
    # a range reads only its own bytes: the files before and after it may be missing
    from vortex_amd import merkle

    _, _, findex, _ = merkle.torrent_pieces(flens, pl)
    mine = {findex[i] for i in range(5, 9)}
    ghost = [p if f in mine else p + ".absent" for f, p in enumerate(paths)]
    got, bad = pool.verify_merkle_files(ghost, flens, pl, exp, first=5, count=4)
    assert (got, bad) == (whole[5:9], 0)


def test_direct_io_and_io_threads_give_the_same_verdicts(built, gpu, torrent):
    from vortex_amd.hash_pool import HashPool

    pl = 1 << 20
    paths, flens, roots, _ = torrent(pl)
    wrong = list(roots)
    wrong[3] = bytes(32)
    exp = b"".join(wrong)
    want = [i != 3 for i in range(len(roots))]
    for direct in (0, 1):
        with HashPool(16384, slots=3, slot_bytes=4 << 20, direct_io=direct) as p:
            for threads in (1, 4):
                got, bad = p.verify_merkle_files(paths, flens, pl, exp, io_threads=threads)
                assert (got, bad) == (want, 0), (direct, threads)
                assert p.last_verify()["readers"] == threads


def test_busy_while_async_pieces_are_pending(pool, torrent):
    from vortex_amd._lib import VX_EBUSY, VxError

    pl = 16384
    paths, flens, roots, _ = torrent(pl)
    body = random_bytes(9, 16384)
    pool.spawn(0, 1, bytearray(body), len(body), hashlib.sha1(body).digest())
    with pytest.raises(VxError) as e:
        pool.verify_merkle_files(paths, flens, pl, b"".join(roots))
    assert e.value.code == VX_EBUSY
    pool.drain()
    r = pool.try_recv()
    assert r.hash_matched
    got, bad = pool.verify_merkle_files(paths, flens, pl, b"".join(roots))
    assert bad == 0 and all(got)
