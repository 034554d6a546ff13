"""Which parts of a torrent's files were never written: the ``os.lseek`` model
of the engine's hole scan (vortex_amd/csrc/vx_extents.hpp).
Host only, no torch, no GPU: what ``HashPool.skip_holes`` makes the re-verify
skip, restated for the tests and tools to compare with.

Hole rule.  With bound = min(the file's size on disk, its torrent length), a
byte is a hole byte iff its offset is below bound and in no data extent
(``SEEK_DATA`` / ``SEEK_HOLE``).  Bytes past the end of a short file are
missing, not holes; a file that does not open has no holes; an lseek error
other than ENXIO makes the whole file data; at most ``cap`` extents are scanned
per file and what lies beyond them is data.
"""
from __future__ import annotations

import errno
import os
from bisect import bisect_right

from . import merkle

MAX_EXTENTS = 65536


def data_extents(path: str, length: int, cap: int = MAX_EXTENTS) -> tuple[int, list[tuple[int, int]]]:
    """(bound, extents) of one file of torrent length ``length``: its sorted
    data extents [lo, hi) clipped to bound.  A file that does not open, or is
    empty, gives (0, []): nothing below the bound, so no holes."""
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return 0, []
    try:
        bound = min(os.fstat(fd).st_size, int(length))
        out: list[tuple[int, int]] = []
        pos = 0
        while pos < bound:
            if len(out) >= cap:  # past the cap: data
                out.append((pos, bound))
                break
            try:
                d = os.lseek(fd, pos, os.SEEK_DATA)
            except OSError as e:
                if e.errno == errno.ENXIO:  # a hole to the end of the file
                    break
                return bound, [(0, bound)]  # the file system does not say: all data
            try:
                h = os.lseek(fd, d, os.SEEK_HOLE)
            except OSError:
                return bound, [(0, bound)]
            if h <= d:
                return bound, [(0, bound)]
            if d >= bound:
                break
            out.append((d, min(h, bound)))
            pos = h
        return bound, out
    finally:
        os.close(fd)


class Holes:
    """The scan of every file of a torrent; ``hole(f, off, len)`` says whether
    bytes [off, off + len) of file f are all hole bytes."""

    def __init__(self, paths, file_lengths, cap: int = MAX_EXTENTS):
        self.files = [data_extents(p, int(n), cap) for p, n in zip(paths, file_lengths)]
        self.extents = sum(len(e) for _, e in self.files)
        self._his = [[hi for _, hi in e] for _, e in self.files]

    def hole(self, f: int, off: int, length: int) -> bool:
        bound, ext = self.files[f]
        if length <= 0 or off < 0 or off + length > bound:
            return False
        k = bisect_right(self._his[f], off)  # the first extent that ends past off
        return k == len(ext) or ext[k][0] >= off + length


def piece_segments(file_lengths, piece_length: int) -> list[list[tuple[int, int, int]]]:
    """v1: per piece, its (file, offset, length) segments over the files laid
    end to end (vx_files::segments; empty files have none)."""
    total = sum(int(n) for n in file_lengths)
    n = (total + piece_length - 1) // piece_length
    segs: list[list[tuple[int, int, int]]] = [[] for _ in range(n)]
    start = 0
    for f, length in enumerate(int(x) for x in file_lengths):
        at = 0
        while at < length:
            i = (start + at) // piece_length
            take = min(length - at, (i + 1) * piece_length - (start + at))
            segs[i].append((f, at, take))
            at += take
        start += length
    return segs


def hole_pieces(paths, file_lengths, piece_length: int, cap: int = MAX_EXTENTS) -> tuple[list[bool], int]:
    """v1 (``verify_files``): (per piece, whether every one of its segments
    lies wholly in holes; the data extents scanned over all files)."""
    holes = Holes(paths, file_lengths, cap)
    segs = piece_segments(file_lengths, piece_length)
    return [bool(s) and all(holes.hole(*x) for x in s) for s in segs], holes.extents


HYBRID_CHUNK = 256 * 1024  # vx_hybrid::kChunk


def hybrid_chunk(piece_length: int, chunk: int | None = None) -> int:
    """The chunk of the hybrid rounds (vx_hybrid::chunk_for on a stage that
    holds a piece): ``chunk``, or the whole piece where a piece is shorter than
    two chunks."""
    c = HYBRID_CHUNK if chunk is None else int(chunk)
    return piece_length if piece_length < 2 * c else c // merkle.BLOCK * merkle.BLOCK


def hole_chunks(paths, file_lengths, piece_length: int, chunk: int | None = None,
                cap: int = MAX_EXTENTS) -> tuple[list[list[bool]], int]:
    """Hybrid (``verify_hybrid_files``): (per piece of ``hybrid.hybrid_pieces``,
    per chunk of it, whether the chunk's data bytes all lie in holes; the data
    extents scanned over all files)."""
    holes = Holes(paths, file_lengths, cap)
    C = hybrid_chunk(piece_length, chunk)
    lens, _, findex, foff = merkle.torrent_pieces(file_lengths, piece_length)
    out = []
    for plen, f, off in zip(lens, findex, foff):
        out.append([holes.hole(f, off + at, min(C, plen - at)) for at in range(0, plen, C)])
    return out, holes.extents


def hybrid_read_bytes(paths, file_lengths, piece_length: int, chunk: int | None = None, first: int = 0,
                      count: int | None = None, cap: int = MAX_EXTENTS) -> dict:
    """What ``verify_hybrid_files`` reads and skips over pieces [first, first +
    count) with ``skip_holes`` on.  Every hole chunk is skipped but those of the
    trailing hole run of the torrent's last piece when that piece is shorter
    than ``piece_length`` (it has no pad, so its v1 total is not the piece
    length and no tail lane can end it) and not wholly a hole: they are read.
    Keys: read_bytes, hole_bytes, hole_blocks, hole_pieces (no byte read),
    zero_runs (hole chunks in front of a data chunk), extents."""
    masks, extents = hole_chunks(paths, file_lengths, piece_length, chunk, cap)
    C = hybrid_chunk(piece_length, chunk)
    lens = merkle.torrent_pieces(file_lengths, piece_length)[0]
    n = len(lens)
    count = n - first if count is None else count
    out = dict(read_bytes=0, hole_bytes=0, hole_blocks=0, hole_pieces=0, zero_runs=0, extents=extents)
    for i in range(first, first + count):
        mask, plen = list(masks[i]), lens[i]
        t = len(mask)  # the trailing hole run is chunks [t, end)
        while t and mask[t - 1]:
            t -= 1
        if 0 < t < len(mask) and i == n - 1 and plen < piece_length:
            mask[t:] = [False] * (len(mask) - t)
        out["hole_pieces"] += t == 0
        out["zero_runs"] += sum(mask[:t])
        for k, hole in enumerate(mask):
            nbytes = min(C, plen - k * C)
            if hole:
                out["hole_bytes"] += nbytes
                out["hole_blocks"] += -(-nbytes // merkle.BLOCK)
            else:
                out["read_bytes"] += nbytes
    return out


def hole_blocks(paths, file_lengths, piece_length: int, cap: int = MAX_EXTENTS) -> tuple[list[list[bool]], int]:
    """v2 (``verify_merkle_files``): (per piece of ``merkle.torrent_pieces``,
    per 16 KiB block of it, whether the block lies wholly in a hole; the data
    extents scanned over all files)."""
    holes = Holes(paths, file_lengths, cap)
    lens, _, findex, foff = merkle.torrent_pieces(file_lengths, piece_length)
    out = []
    for plen, f, off in zip(lens, findex, foff):
        out.append([holes.hole(f, off + at, min(merkle.BLOCK, plen - at)) for at in range(0, plen, merkle.BLOCK)])
    return out, holes.extents
