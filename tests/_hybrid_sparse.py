"""Shared by the hybrid file-hole tests (test_hybrid_sparse_cpu.py,
test_gpu_hybrid_sparse.py): hybrid torrents whose files were written chunk by
chunk, every way a crash can leave them, and what hashlib says of them.

A torrent is a dict: name, pl, paths, flens, content (per file, the bytes the
file holds over its torrent length, zeros where nothing was written), disk (per
file, its size on disk: bytes past it are missing), exp1 / exp2 (the expected
SHA-1 rows and roots, some damaged) and want (per piece, the verdict byte
hashlib gives: bit 0 SHA-1, bit 1 root, 0 for a piece that lacks bytes).
Nothing here reads the files back: a fallocated range that has been read
through the page cache can report as data afterwards."""
import hashlib
import random

from _sparse import make_file

BLOCK = 16384
PL = 1 << 20
C = 256 << 10
TAIL = 3 * BLOCK + 37  # what a file-end piece holds past its whole chunks


def chunked_file(path, length, unwritten, rng, how="truncate", chunk=C, size=None, punch=()):
    """A file of `length` random bytes made by `how`, written chunk by chunk but
    for the chunks in `unwritten`; punch: (offset, length) ranges inside written
    chunks that are left out of the writes too.  Returns (path, content)."""
    content = bytearray(rng.randbytes(length))
    writes = []
    for j in range(-(-length // chunk)):
        lo, hi = j * chunk, min((j + 1) * chunk, length)
        if j in unwritten:
            content[lo:hi] = bytes(hi - lo)
            continue
        at = lo
        for off, n in sorted(p for p in punch if lo <= p[0] < hi):
            writes.append((at, bytes(content[at:off])))
            content[off:off + n] = bytes(n)
            at = off + n
        writes.append((at, bytes(content[at:hi])))
    make_file(path, length, writes=[w for w in writes if w[1]], how=how, size=size)
    return str(path), bytes(content)


def _bits(mask, n):
    return {j for j in range(n) if mask >> j & 1}


def _finish(name, pl, files, disk=None, bad1=(), bad2=()):
    from vortex_amd import hybrid

    paths = [p for p, _ in files]
    content = [c for _, c in files]
    flens = [len(c) for c in content]
    disk = list(disk) if disk else list(flens)
    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(flens, pl)
    exp1, exp2, want = bytearray(), bytearray(), []
    for i, (f, o, n, pad, lw) in enumerate(zip(findex, foff, dlen, pads, log2w)):
        data = content[f][o:o + n]
        d1, d2 = bytearray(hybrid.v1_digest(data, pad)), bytearray(hybrid.v2_root(data, lw))
        if i in bad1:
            d1[i % 20] ^= 1 << (i % 8)
        if i in bad2:
            d2[i % 32] ^= 1 << (i % 8)
        exp1 += d1
        exp2 += d2
        want.append(0 if o + n > disk[f] else (i not in bad1) | (i not in bad2) << 1)
    return dict(name=name, pl=pl, paths=paths, flens=flens, content=content, disk=disk, exp1=bytes(exp1),
                exp2=bytes(exp2), want=want, io_errors=sum(o + n > disk[f] for f, o, n in zip(findex, foff, dlen)))


def main_torrent(d, seed=5):
    """1 MiB pieces.  File 0: 16 full pieces, chunk j of piece m unwritten iff
    bit j of m.  Then, for k in 0..3, one file of k C + TAIL bytes per hole mask
    over its k + 1 chunks (30 files, each followed by an implied pad): pieces 16
    to 45.  Last, one full piece with a 16 KiB hole inside a written chunk:
    piece 46, which is read whole.  The all-hole pieces are 15, 17, 21, 29, 45."""
    rng = random.Random(seed)
    files = [chunked_file(d / "m0", 16 * PL, {4 * m + j for m in range(16) for j in _bits(m, 4)}, rng)]
    for k in range(4):
        for mask in range(1 << (k + 1)):
            files.append(chunked_file(d / f"e{k}_{mask}", k * C + TAIL, _bits(mask, k + 1), rng,
                                      how="fallocate" if mask % 3 == 1 else "truncate"))
    files.append(chunked_file(d / "punched", PL, set(), rng, punch=[(C + 2 * BLOCK, BLOCK)]))
    # hole pieces whose SHA-1 row is wrong and whose root is right (15, 29), the reverse (21), both (33: a
    # trailing hole); and rows of pieces with data, with a leading (1), middle (5, 10) or trailing (8) hole
    return _finish("main", PL, files, bad1={0, 5, 8, 15, 29, 33}, bad2={1, 10, 21, 33, 40})


def last_piece_torrents(d, seed=6):
    """Three torrents of one file, a full piece and a short unpadded last piece
    of 2 C + 5,000 bytes (three chunks): its trailing chunk a hole (which must be
    read), the whole piece a hole, its leading chunk a hole."""
    out = []
    for name, unwritten, bad1 in (("last-trailing", {6}, ()), ("last-whole", {4, 5, 6}, ()), ("last-leading", {0, 4}, (1,))):
        rng = random.Random(seed + len(out))
        sub = d / name
        sub.mkdir()
        out.append(_finish(name, PL, [chunked_file(sub / "f", PL + 2 * C + 5000, unwritten, rng)], bad1=set(bad1)))
    return out


def short_on_disk_torrent(d, seed=9):
    """A file of three pieces that is 1 MiB + 2 C on disk, with holes below its
    size, and a written file behind it: piece 0 has its first chunk only, piece 1
    a hole and a written chunk and lacks the rest, piece 2 lacks everything."""
    rng = random.Random(seed)
    sub = d / "short"
    sub.mkdir()
    files = [chunked_file(sub / "a", 3 * PL, {1, 2, 3, 4, 6, 7, 8, 9, 10, 11}, rng, size=PL + 2 * C),
             chunked_file(sub / "b", C + 100, set(), rng)]
    return _finish("short-on-disk", PL, files, disk=[PL + 2 * C, C + 100])


def small_piece_torrent(d, seed=10):
    """256 KiB pieces: one chunk per piece, so only whole pieces are holes.  A
    file of 11 pieces and 100,000 bytes (a padded piece), then a short file."""
    rng = random.Random(seed)
    sub = d / "small"
    sub.mkdir()
    files = [chunked_file(sub / "a", 11 * C + 100_000, {1, 2, 5, 6, 7, 10, 11}, rng, how="fallocate"),
             chunked_file(sub / "b", 70_000, {0}, rng)]
    return _finish("256KiB", C, files, bad1={2, 4, 11}, bad2={6, 12})


def all_torrents(d):
    """Every torrent above, under directory d; under 64 MiB of file length."""
    out = [main_torrent(d)] + last_piece_torrents(d) + [short_on_disk_torrent(d), small_piece_torrent(d)]
    assert sum(sum(t["flens"]) for t in out) < 64 << 20
    return out


def zero_verdicts(t):
    """The pieces of torrent t whose data is all zeros: (piece, verdict wanted)."""
    from vortex_amd import hybrid

    findex, foff, dlen, _, _ = hybrid.hybrid_pieces(t["flens"], t["pl"])
    return [(i, t["want"][i]) for i, (f, o, n) in enumerate(zip(findex, foff, dlen))
            if not any(t["content"][f][o:o + n]) and o + n <= t["disk"][f]]


def sha1_of_zeros(n):
    return hashlib.sha1(bytes(n)).digest()
