"""GPU: the re-verify over file holes (HashPool.skip_holes).

Pieces (v1) and 16 KiB blocks (v2) the file system never wrote are judged
without a read: the verdicts must be those of the setting off and of hashlib
over the files' real bytes, the hole counts and read_bytes those of the
os.lseek model (vortex_amd/sparse.py), and the zero hashes the kernels make
from nothing those of hashlib.

Every test makes its verdict assertions first and then probes its tmp_path:
where the file system reports no holes the count assertions do not apply."""
import hashlib
import random

import pytest

from _sparse import NO_HOLES, holes_reported, make_file, write_torrent_range

pytestmark = pytest.mark.gpu

BLOCK = 16384
ZERO_LENS = [1, 55, 56, 63, 64, 119, 120, 128, 16384, 65537, 262144]


def test_sha1_zeros_against_hashlib(built, gpu):
    """Lengths on every side of the padding's edges (55 | 56, 63 | 64, 119 |
    120), long ones, all mixed in one wave; then 65 lanes (two waves)."""
    from vortex_amd import device as vdev

    for lens in (ZERO_LENS, [ZERO_LENS[(7 * k) % len(ZERO_LENS)] for k in range(65)]):
        got = vdev.sha1_zeros(lens).cpu().numpy().tobytes()
        assert len(got) == 20 * len(lens)
        for k, n in enumerate(lens):
            assert got[20 * k:20 * k + 20] == hashlib.sha1(bytes(n)).digest(), (k, n)
    assert vdev.sha1_zeros([]).shape == (0, 20)
    with pytest.raises(ValueError):
        vdev.sha1_zeros([-1])
    with pytest.raises(ValueError):
        vdev.sha1_zeros([1 << 32])


def test_merkle_zero_leaves_against_hashlib(built, gpu):
    import torch

    from vortex_amd import device as vdev

    lens = [1, 55, 56, 63, 64, 16383, 16384]
    got = vdev.merkle_zero_leaves(lens).cpu().numpy().tobytes()
    for k, n in enumerate(lens):
        assert got[32 * k:32 * k + 32] == hashlib.sha256(bytes(n)).digest(), (k, n)
    # a device tensor of lengths, more than one workgroup
    many = [lens[(5 * k) % len(lens)] for k in range(300)]
    got = vdev.merkle_zero_leaves(torch.tensor(many, dtype=torch.int32, device=gpu)).cpu().numpy().tobytes()
    assert got == b"".join(hashlib.sha256(bytes(n)).digest() for n in many)
    assert vdev.merkle_zero_leaves([]).shape == (0, 32)
    for bad in ([0], [16385]):
        with pytest.raises(ValueError):
            vdev.merkle_zero_leaves(bad)


def _v1_case(tmp_path, pl, sizes, written, zeros, zero_expected, seed, short=None):
    """Files of `sizes` truncated to length; torrent pieces `written` written
    with data, pieces `zeros` written as real zero bytes, pieces
    `zero_expected` left unwritten with an expected row that is the zero
    digest (the torrent's content there is zeros).  short = (file, size): that
    file is cut to size on disk afterwards.  Returns (paths, expected table,
    the verdicts hashlib gives over what the files hold)."""
    rng = random.Random(seed)
    data = bytearray(rng.getrandbits(8) for _ in range(sum(sizes)))
    n = (len(data) + pl - 1) // pl
    for i in set(zeros) | set(zero_expected):
        data[i * pl:(i + 1) * pl] = bytes(len(data[i * pl:(i + 1) * pl]))
    exp = b"".join(hashlib.sha1(bytes(data[i * pl:(i + 1) * pl])).digest() for i in range(n))
    paths = [make_file(tmp_path / f"f{k}", L) for k, L in enumerate(sizes)]
    for i in sorted(set(written) | set(zeros)):
        write_torrent_range(paths, sizes, i * pl, min((i + 1) * pl, len(data)), bytes(data))
    if short:
        with open(paths[short[0]], "r+b") as f:
            f.truncate(short[1])
    held = b"".join(open(p, "rb").read().ljust(L, b"\xff")[:L] for p, L in zip(paths, sizes))
    lacking = bytearray(len(held))  # bytes past a short file's end are missing: the piece fails
    acc = 0
    for k, (p, L) in enumerate(zip(paths, sizes)):
        if short and k == short[0]:
            lacking[acc + short[1]:acc + L] = b"\x01" * (L - short[1])
        acc += L
    want = [hashlib.sha1(held[i * pl:(i + 1) * pl]).digest() == exp[20 * i:20 * i + 20]
            and not any(lacking[i * pl:(i + 1) * pl]) for i in range(n)]
    return paths, exp, want


def _piece_len(i, pl, total):
    return min(pl, total - i * pl)


def test_v1_whole_piece_path(built, gpu, tmp_path):
    """The layout of test_fresh_fallocated_files: 64 KiB pieces over files of
    100,000 / 3 pl + 5 / 17 / 2 pl bytes; two pieces written, one written as
    real zeros, the last (short) one unwritten with the zero digest expected."""
    from vortex_amd import sparse
    from vortex_amd.hash_pool import HashPool

    pl = 64 * 1024
    sizes = [100_000, 3 * pl + 5, 17, 2 * pl]
    total, n = sum(sizes), (sum(sizes) + pl - 1) // pl
    paths, exp, want = _v1_case(tmp_path, pl, sizes, written={0, 3}, zeros={2}, zero_expected={n - 1}, seed=1)
    holes, extents = sparse.hole_pieces(paths, sizes, pl)
    with HashPool(pl) as pool:
        assert pool.skip_holes is False
        pool.skip_holes = True
        on = pool.verify_files(paths, sizes, pl, exp)
        trace, read_on = pool.last_verify_holes(), pool.last_verify()["read_bytes"]
        stats_on = pool.stats()
        again = pool.verify_files(paths, sizes, pl, exp)
        trace2 = pool.last_verify_holes()
        pool.skip_holes = False
        pool.reset_stats()
        off = pool.verify_files(paths, sizes, pl, exp)
        assert pool.last_verify_holes() == dict.fromkeys(trace, 0)
        stats_off = pool.stats()
    assert on == off == again == (want, 0)
    assert want == [True, False, True, True, False, False, True]
    for key in ("pieces_completed", "pieces_mismatched", "bytes_completed", "io_errors"):
        assert stats_on[key] == stats_off[key], key
    assert trace2["zero_hash_ms"] == 0  # the digest came from the context's cache
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    assert holes[n - 1] and sum(holes) >= 1 and not holes[0] and not holes[2] and not holes[3]
    assert trace["hole_pieces"] == sum(holes) == trace2["hole_pieces"] and trace["extents"] == extents
    assert trace["hole_bytes"] == sum(_piece_len(i, pl, total) for i in range(n) if holes[i])
    assert read_on == total - trace["hole_bytes"]
    assert trace["hole_blocks"] == 0 and trace["zero_hash_ms"] > 0 and trace["scan_ms"] > 0


def test_v1_chunk_path(built, gpu, tmp_path):
    """256 KiB pieces in 64 KiB chunk rounds; the short last piece (64,056
    bytes: 56 mod 64) is a hole; range calls that start and end inside hole
    runs; a call whose pieces are all holes."""
    from vortex_amd import sparse
    from vortex_amd.hash_pool import HashPool

    pl, last = 256 * 1024, 1000 * 64 + 56
    sizes = [5 * pl + 4096, 4 * pl - 4096 + last]
    total, n = sum(sizes), 10
    # piece 5 spans both files (at a 4 KiB boundary of each, so its neighbours stay unwritten); 7 is
    # written as zeros; 3 and the last are unwritten zeros of the torrent
    paths, exp, want = _v1_case(tmp_path, pl, sizes, written={1, 5}, zeros={7}, zero_expected={3, n - 1}, seed=2)
    holes, extents = sparse.hole_pieces(paths, sizes, pl)
    ranges = [(0, n), (2, 3), (3, 6), (8, 2)]
    got = {}
    with HashPool(pl, slots=3, batch_pieces=4, slot_bytes=4 << 20, verify_chunk=65536) as pool:
        for skip in (True, False):
            pool.skip_holes = skip
            for first, count in ranges:
                pool.reset_stats()
                rounds0 = pool.stats()["chunk_rounds"]
                res = pool.verify_files(paths, sizes, pl, exp, io_threads=3, first=first, count=count)
                st = pool.stats()
                got[skip, first, count] = (res, pool.last_verify_holes(), pool.last_verify()["read_bytes"],
                                           st["chunk_rounds"] - rounds0,
                                           (st["pieces_completed"], st["pieces_mismatched"], st["bytes_completed"]))
    for first, count in ranges:
        on, off = got[True, first, count], got[False, first, count]
        assert on[0] == off[0] == (want[first:first + count], 0), (first, count)
        assert on[4] == off[4], (first, count)
    assert want == [False, True, False, True, False, True, False, True, False, True]
    assert got[False, 0, n][3] >= 4  # the chunk path ran: a piece takes pl / chunk rounds
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    assert [i for i in range(n) if holes[i]] == [0, 2, 3, 4, 6, 8, 9]
    for first, count in ranges:
        _, trace, read_bytes, rounds, _ = got[True, first, count]
        mine = [i for i in range(first, first + count) if holes[i]]
        assert trace["hole_pieces"] == len(mine) and trace["extents"] == extents
        assert trace["hole_bytes"] == sum(_piece_len(i, pl, total) for i in mine)
        assert read_bytes == sum(_piece_len(i, pl, total) for i in range(first, first + count)) - trace["hole_bytes"]
        if len(mine) == count:  # every piece a hole: no round, nothing read
            assert rounds == 0 and read_bytes == 0
    assert got[True, 2, 3][3] == 0 and got[True, 8, 2][3] == 0
    # the first call made both digests (piece length and last piece); every later one found them cached
    assert got[True, 0, n][1]["zero_hash_ms"] > 0
    assert all(got[True, f, c][1]["zero_hash_ms"] == 0 for f, c in ranges[1:])


def test_v1_short_file_and_holes(built, gpu, tmp_path):
    """A file shorter on disk than its torrent length, among holes: bytes past
    its end are missing, not holes, so the failed pieces and the count of I/O
    errors are those of the setting off."""
    from vortex_amd import sparse
    from vortex_amd.hash_pool import HashPool

    pl = 64 * 1024
    sizes = [100_000, 3 * pl + 5, 17, 2 * pl]
    total, n = sum(sizes), (sum(sizes) + pl - 1) // pl
    paths, exp, want = _v1_case(tmp_path, pl, sizes, written={0}, zeros=set(), zero_expected={1, 2, 5, 6}, seed=3,
                                short=(3, pl // 2))
    holes, _ = sparse.hole_pieces(paths, sizes, pl)
    with HashPool(pl) as pool:
        pool.skip_holes = True
        on = pool.verify_files(paths, sizes, pl, exp)
        trace = pool.last_verify_holes()
        pool.skip_holes = False
        off = pool.verify_files(paths, sizes, pl, exp)
    assert on == off and on[0] == want
    assert on[1] == 2 and want[5:] == [False, False] and want[1] and want[2]  # the two pieces past f3's end
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    assert holes[1] and holes[2] and not holes[5] and not holes[6]
    assert trace["hole_pieces"] == sum(holes)


def test_v2_blocks(built, gpu, tmp_path):
    """64 KiB pieces (four blocks): a piece with two written and two hole
    blocks, an all-hole piece against the zero-content root, a short file wholly
    a hole, a file whose short last block is a hole, a damaged written block."""
    from vortex_amd import hybrid, merkle, sparse
    from vortex_amd.hash_pool import HashPool

    pl = 64 * 1024
    rng = random.Random(4)
    flens = [2 * pl, 20_000, pl + 5_000, 2 * pl]
    body = [bytearray(rng.getrandbits(8) for _ in range(n)) for n in flens]
    body[0][:BLOCK] = bytes(BLOCK)               # file a, piece 0: blocks 0 and 3 are zeros of the torrent,
    body[0][3 * BLOCK:] = bytes(pl + BLOCK)      # ... and piece 1 is all zeros
    body[1][:] = bytes(flens[1])
    body[2][pl:] = bytes(5_000)
    paths = [
        make_file(tmp_path / "a", flens[0], writes=[(BLOCK, bytes(body[0][BLOCK:3 * BLOCK]))]),
        make_file(tmp_path / "b", flens[1], how="fallocate"),
        make_file(tmp_path / "c", flens[2], writes=[(0, bytes(body[2][:pl]))]),
        make_file(tmp_path / "d", flens[3], writes=[(0, bytes(body[3]))]),
    ]
    lens, log2w, findex, foff = merkle.torrent_pieces(flens, pl)
    exp = b"".join(hybrid.v2_root(bytes(body[f][o:o + n]), w) for n, w, f, o in zip(lens, log2w, findex, foff))
    with open(paths[3], "r+b") as f:  # damage a written block of d's second piece
        f.seek(pl + BLOCK + 7)
        f.write(bytes([body[3][pl + BLOCK + 7] ^ 0x10]))
    hb, extents = sparse.hole_blocks(paths, flens, pl)  # (before anything reads the fallocated file)
    with HashPool(pl) as pool:
        pool.skip_holes = True
        on = pool.verify_merkle_files(paths, flens, pl, exp)
        trace, read_on = pool.last_verify_holes(), pool.last_verify()["read_bytes"]
        sub = pool.verify_merkle_files(paths, flens, pl, exp, first=1, count=3)
        trace_sub = pool.last_verify_holes()
        pool.skip_holes = False
        off = pool.verify_merkle_files(paths, flens, pl, exp)
        assert pool.last_verify_holes() == dict.fromkeys(trace, 0)
    real = [open(p, "rb").read() for p in paths]
    want = [hybrid.v2_root(real[f][o:o + n], w) == exp[32 * i:32 * i + 32]
            for i, (n, w, f, o) in enumerate(zip(lens, log2w, findex, foff))]
    assert want == [True, True, True, True, True, True, False]
    assert on == off == (want, 0) and sub == (want[1:4], 0)
    assert trace_sub["zero_hash_ms"] == 0  # the full block's row came from the context
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    assert hb[:5] == [[True, False, False, True], [True] * 4, [True, True], [False] * 4, [True]]
    hole_bytes = sum(min(BLOCK, n - k * BLOCK) for n, blocks in zip(lens, hb) for k, h in enumerate(blocks) if h)
    assert trace["hole_blocks"] == sum(map(sum, hb)) == 9 and trace["hole_bytes"] == hole_bytes
    assert trace["extents"] == extents and trace["hole_pieces"] == 0 and trace["zero_hash_ms"] > 0
    assert read_on == sum(flens) - hole_bytes == 2 * BLOCK + pl + 2 * pl  # the written blocks' bytes
    assert trace_sub["hole_blocks"] == sum(map(sum, hb[1:4]))
