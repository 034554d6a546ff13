"""Hybrid (BEP 52 "upgrade path", v1 + v2) piece geometry: host-only, no torch.

A hybrid torrent carries a v1 ``pieces`` table and v2 ``piece layers`` /
``pieces root`` rows over one set of files.  Every file but the last is padded
to a piece boundary with a BEP 47 pad file (``attr = p``, all zeros), so every
file starts its own pieces in v1 as it does in v2: v1 piece i is v2 piece i
(:func:`merkle.torrent_pieces`'s numbering), and the v1 piece that ends a file
is the file's bytes followed by zeros up to ``piece_length``.  The torrent's
last piece is not padded.  Clients do not write pad files; the engine hashes
the zeros without reading them (``HashPool.verify_hybrid_files``,
``device.hybrid_pieces``).
"""
from __future__ import annotations

import hashlib

from . import merkle


def hybrid_pieces(file_lengths, piece_length: int) -> tuple[list[int], list[int], list[int], list[int], list[int]]:
    """(file_index, file_offset, data_len, pad_len, log2w) of every piece of a
    hybrid torrent, in torrent order; ``file_lengths`` lists the real files
    only (no pad files).  Piece i is bytes [file_offset[i], file_offset[i] +
    data_len[i]) of file file_index[i]; its v1 digest is over those bytes
    followed by pad_len[i] zeros, its v2 root over the bytes alone as a tree of
    2^log2w[i] leaf slots.  pad_len = piece_length - data_len for a file's
    short last piece, except the torrent's last piece (the last piece of the
    last non-empty file), which v1 does not pad.  Empty files have no pieces."""
    lens, log2w, file_index, file_offset = merkle.torrent_pieces(file_lengths, piece_length)
    n = len(lens)
    pads = [piece_length - L if L < piece_length and i != n - 1 else 0 for i, L in enumerate(lens)]
    return file_index, file_offset, lens, pads, log2w


def v1_digest(data, pad_len: int = 0) -> bytes:
    """SHA-1 of data followed by pad_len zero bytes (hashlib): the v1 `pieces`
    entry of a hybrid piece."""
    if pad_len < 0:
        raise ValueError("pad_len must be >= 0")
    h = hashlib.sha1(bytes(data))
    zeros = bytes(min(pad_len, 1 << 20))
    left = pad_len
    while left:
        k = min(left, len(zeros))
        h.update(zeros[:k])
        left -= k
    return h.digest()


def v2_root(data, log2w: int) -> bytes:
    """Merkle root of a piece (hashlib): SHA-256 leaves over 16 KiB blocks, 2^log2w
    leaf slots, the slots past the data all-zero rows."""
    data = bytes(data)
    rows = [hashlib.sha256(data[o:o + merkle.BLOCK]).digest() if o < len(data) else bytes(32)
            for o in range(0, merkle.BLOCK << log2w, merkle.BLOCK)]
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]
