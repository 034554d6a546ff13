"""BitTorrent v2 (BEP 52) piece geometry: host-only helpers, no torch, no GPU.

A v2 piece is verified as a SHA-256 merkle tree over 16 KiB blocks
(include/vx_hash.h, "BitTorrent v2").  These helpers say, for one file of a
torrent, which pieces it has and how wide each piece's tree is: the lengths
and ``log2w`` that ``device.merkle_ragged`` and ``HashPool.verify_merkle``
take.
"""
from __future__ import annotations

import hashlib

BLOCK = 16384  # VX_MERKLE_BLOCK
MAX_LOG2_WIDTH = 17  # VX_MERKLE_MAX_LOG2_WIDTH


def log2_width(piece_length: int) -> int:
    """log2 of the leaf slots of a piece_length-byte piece."""
    if piece_length < BLOCK or piece_length & (piece_length - 1):
        raise ValueError("piece_length must be a power of two >= 16384")
    w = (piece_length // BLOCK).bit_length() - 1
    if w > MAX_LOG2_WIDTH:
        raise ValueError("piece_length above 2 GiB")
    return w


def file_pieces(file_length: int, piece_length: int) -> tuple[list[int], list[int]]:
    """(lens, log2w) of the pieces of one file.

    A file longer than piece_length has ceil(file_length / piece_length)
    pieces, each (the short last one included) a tree of piece_length / 16 KiB
    leaf slots; their roots are the file's `piece layers` entry.  A file of at
    most piece_length bytes is one piece whose tree is as wide as its block
    count rounded up to a power of two; its root is the file's `pieces root`.
    An empty file has no pieces."""
    full = log2_width(piece_length)
    if file_length < 0:
        raise ValueError("file_length must be >= 0")
    if file_length == 0:
        return [], []
    if file_length <= piece_length:
        blocks = (file_length + BLOCK - 1) // BLOCK
        return [file_length], [(blocks - 1).bit_length()]
    n = (file_length + piece_length - 1) // piece_length
    lens = [piece_length] * (n - 1) + [file_length - (n - 1) * piece_length]
    return lens, [full] * n


def torrent_pieces(file_lengths, piece_length: int) -> tuple[list[int], list[int], list[int], list[int]]:
    """(lens, log2w, file_index, file_offset) of every piece of a torrent:
    :func:`file_pieces` file after file, in the order given.  Every file starts
    its own pieces and no piece spans files; an empty file has none.  This is
    the numbering ``HashPool.verify_merkle_files`` and its ``expected`` table
    use: piece i is file_lengths[file_index[i]] bytes
    [file_offset[i], file_offset[i] + lens[i])."""
    lens: list[int] = []
    log2w: list[int] = []
    file_index: list[int] = []
    file_offset: list[int] = []
    for f, length in enumerate(file_lengths):
        fl, fw = file_pieces(int(length), piece_length)
        lens += fl
        log2w += fw
        file_index += [f] * len(fl)
        file_offset += [k * piece_length for k in range(len(fl))]
    return lens, log2w, file_index, file_offset


def pad_hash(height: int) -> bytes:
    """pad(0) = 32 zero bytes; pad(h) = SHA-256(pad(h-1) || pad(h-1)): the root
    of an all-zero subtree of 2^height leaves (vx_merkle_pad_hash)."""
    if height < 0:
        raise ValueError("height must be >= 0")
    h = bytes(32)
    for _ in range(height):
        h = hashlib.sha256(h + h).digest()
    return h
