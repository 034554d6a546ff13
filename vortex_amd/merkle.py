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


def _rows(hashes) -> list[bytes]:
    """A layer as a list of 32-byte rows: bytes-like (n * 32) or a sequence of rows."""
    if isinstance(hashes, (bytes, bytearray, memoryview)):
        b = bytes(hashes)
        if len(b) % 32:
            raise ValueError("a layer holds whole 32-byte hashes")
        return [b[k:k + 32] for k in range(0, len(b), 32)]
    rows = [bytes(r) for r in hashes]
    if any(len(r) != 32 for r in rows):
        raise ValueError("a layer holds whole 32-byte hashes")
    return rows


def layer_counts(file_lengths, piece_length: int) -> tuple[list[int], list[int]]:
    """(counts, file_index) of a torrent's `piece layers`: one layer per file
    longer than piece_length, ceil(length / piece_length) hashes each, in the
    order given.  A shorter file has no layer: its one piece's root is its
    `pieces root` itself.  counts is what ``device.merkle_layers`` takes."""
    log2_width(piece_length)
    counts: list[int] = []
    file_index: list[int] = []
    for f, length in enumerate(file_lengths):
        if int(length) > piece_length:
            counts.append((int(length) + piece_length - 1) // piece_length)
            file_index.append(f)
    return counts, file_index


class _Tree:
    """The BEP 52 tree over a layer standing `height` levels above the leaves:
    node (j, i) is row i of the layer at level 0, the pad hash of its height
    where its whole subtree lies past the layer, and SHA-256(left || right)
    otherwise."""

    def __init__(self, rows: list[bytes], height: int):
        self.levels = [rows]
        self.height = height

    def node(self, j: int, i: int) -> bytes:
        n = len(self.levels[0])
        if (i << j) >= n:
            return pad_hash(self.height + j)
        while len(self.levels) <= j:
            below = len(self.levels) - 1
            count = (n + (2 << below) - 1) >> (below + 1)
            self.levels.append([hashlib.sha256(self.node(below, 2 * k) + self.node(below, 2 * k + 1)).digest()
                                for k in range(count)])
        return self.levels[j][i]


def layer_root(hashes, height: int = 0) -> bytes:
    """Root of a layer of n >= 1 hashes standing `height` levels above the
    leaves: padded to the next power of two with pad_hash(height), then reduced
    pairwise (how a `piece layers` string is checked against `pieces root`;
    vx_merkle_device_root and vx_merkle_device_layers compute the same)."""
    rows = _rows(hashes)
    if not rows:
        raise ValueError("a layer holds at least one hash")
    return _Tree(rows, height).node((len(rows) - 1).bit_length(), 0)


def tree_rows(m: int) -> int:
    """Rows of the tree of an m-row layer (vx_merkle_tree_rows): level k holds
    ceil(m / 2^k) rows, k = 0..ceil(log2 m); 0 for m = 0."""
    if m < 0:
        raise ValueError("m must be >= 0")
    if m == 0:
        return 0
    return sum((m + (1 << k) - 1) >> k for k in range((m - 1).bit_length() + 1))


def tree_layout(file_lengths, piece_length: int) -> tuple[list[int], list[int]]:
    """(counts, tree_off) of a torrent's trees (vx_merkle_tree_layout): per file
    the rows of its layer (0: empty, 1: at most piece_length bytes, the row is
    its `pieces root`; else its piece count) and len(file_lengths) + 1 row
    offsets; file f's tree is rows [tree_off[f], tree_off[f + 1])."""
    log2_width(piece_length)
    counts = [(int(length) + piece_length - 1) // piece_length for length in file_lengths]
    off = [0]
    for c in counts:
        off.append(off[-1] + tree_rows(c))
    return counts, off


def build_tree(rows, height: int = 0) -> bytes:
    """The tree of a layer of m >= 1 hashes standing `height` levels above the
    leaves, with hashlib: every level k = 0..ceil(log2 m), level k the
    ceil(m / 2^k) nodes of the BEP 52 tree that cover a row of the layer (node
    (k, j) of :class:`_Tree`), level 0 first; tree_rows(m) * 32 bytes, the last
    row the layer's root.  The model of vx_merkle_device_trees."""
    level = _rows(rows)
    if not level:
        raise ValueError("a layer holds at least one hash")
    out = [b"".join(level)]
    k = 0
    while len(level) > 1:
        if len(level) & 1:
            level = level + [pad_hash(height + k)]
        level = [hashlib.sha256(level[j] + level[j + 1]).digest() for j in range(0, len(level), 2)]
        out.append(b"".join(level))
        k += 1
    return b"".join(out)


def proof_from_tree(tree: bytes, m: int, height: int, level: int, pos: int, span: int, uncles: int) -> bytes:
    """:func:`make_proof` over level `level` of a layer whose tree is at hand
    (vx_merkle_tree_proof): a lookup that hashes nothing.  Equal to
    make_proof(rows of that level, height + level, pos, span, uncles)."""
    import ctypes

    from ._lib import check, lib

    if len(tree) != 32 * tree_rows(m):
        raise ValueError("tree must hold tree_rows(m) rows of 32 bytes")
    if min(level, pos, span, uncles, height) < 0:
        raise ValueError("level, pos, span, uncles and height must be >= 0")
    out = ctypes.create_string_buffer(32 * (span + uncles) or 1)
    check(lib().vx_merkle_tree_proof(bytes(tree), m, height, level, pos, span, uncles, out), "vx_merkle_tree_proof")
    return out.raw[:32 * (span + uncles)]


def make_proof(layer, height: int, pos: int, span: int, uncles: int) -> bytes:
    """The rows a seeder sends in a `hashes` message for span number `pos` of
    `span` hashes (a power of two) of `layer`: the span's rows
    [pos * span, (pos + 1) * span), then `uncles` uncle hashes, the sibling at
    each step from the span's root upwards.  The layer is padded with
    pad_hash(height), and the levels above with their own pad hashes, as far
    as the proof reaches.  (span + uncles) * 32 bytes, the layout of
    ``vx_merkle_proof``: with uncles = log2(padded layer / span) the walk ends at
    the layer's root, with fewer at an ancestor."""
    if span < 1 or span & (span - 1):
        raise ValueError("span must be a power of two")
    if pos < 0 or uncles < 0:
        raise ValueError("pos and uncles must be >= 0")
    tree = _Tree(_rows(layer), height)
    out = [tree.node(0, pos * span + k) for k in range(span)]
    base = span.bit_length() - 1
    out += [tree.node(base + k, (pos >> k) ^ 1) for k in range(uncles)]
    return b"".join(out)


def bitmap_words(n: int, log2_width: int) -> int:
    """uint64 words of the bad-block bitmap of n pieces of 2^log2_width leaf
    slots (vx_merkle_bitmap_words): max(1, 2^log2_width / 64) per piece; block b
    of piece i is bit b & 63 of word i * wpp + (b >> 6).  0 for a width above
    MAX_LOG2_WIDTH."""
    if n < 0 or log2_width < 0:
        raise ValueError("n and log2_width must be >= 0")
    if log2_width > MAX_LOG2_WIDTH:
        return 0
    return n * max(1, (1 << log2_width) // 64)


def leaf_rows(data, log2w: int) -> bytes:
    """The leaf layer of one piece as a tree of 2^log2w slots, with hashlib:
    SHA-256 of each 16 KiB block (the last at its real length), zero rows for
    the slots at or past the piece's end; (32 << log2w) bytes.  What
    ``device.merkle_block_check`` and ``HashPool.check_blocks`` return."""
    data = bytes(data)
    if not 0 <= log2w <= MAX_LOG2_WIDTH:
        raise ValueError("log2w must be 0..17")
    if len(data) > BLOCK << log2w:
        raise ValueError("the piece is longer than its tree (16384 << log2w bytes)")
    return b"".join(hashlib.sha256(data[o:o + BLOCK]).digest() if o < len(data) else bytes(32)
                    for o in range(0, BLOCK << log2w, BLOCK))


def bad_blocks(data, expected_leaves) -> list[int]:
    """The blocks of one piece whose SHA-256 differs from their row of
    expected_leaves (the piece's 2^log2w leaf rows): the model of the
    bad-block bitmap.  A slot at or past the piece's end is never bad,
    whatever its expected row holds."""
    data = bytes(data)
    rows = _rows(expected_leaves)
    if len(data) > BLOCK * len(rows):
        raise ValueError("the piece is longer than its expected leaf rows")
    return [b for b in range((len(data) + BLOCK - 1) // BLOCK)
            if hashlib.sha256(data[b * BLOCK:(b + 1) * BLOCK]).digest() != rows[b]]


def leaf_layout(file_lengths, piece_length: int) -> tuple[list[int], list[int], int]:
    """(leaf_first, blocks, rows) of a torrent's leaf table (vx_hash.h, "Block
    checks from disk"): the files' leaf layers back to back in file order, file
    f contributing ceil(len_f / 16 KiB) rows, with no padding row anywhere.
    Piece i (the numbering of :func:`torrent_pieces`) has blocks[i] rows from
    row leaf_first[i] on; rows is the whole table's count
    (vx_merkle_leaf_rows)."""
    width = 1 << log2_width(piece_length)
    leaf_first: list[int] = []
    blocks: list[int] = []
    off = 0
    for length in file_lengths:
        lens, _ = file_pieces(int(length), piece_length)
        leaf_first += [off + j * width for j in range(len(lens))]
        blocks += [(n + BLOCK - 1) // BLOCK for n in lens]
        off += (int(length) + BLOCK - 1) // BLOCK
    return leaf_first, blocks, off


def file_leaf_table(paths, file_lengths, piece_length: int) -> bytes:
    """The leaf table of a torrent's files with hashlib: SHA-256 of every 16
    KiB block of every file (a file's last block at its real length), laid out
    by :func:`leaf_layout`.  The model of ``HashPool.hash_merkle_files_leaves``
    and what ``HashPool.verify_merkle_files_blocks`` takes."""
    log2_width(piece_length)
    out = []
    for path, length in zip(paths, file_lengths):
        with open(path, "rb") as f:
            for o in range(0, int(length), BLOCK):
                out.append(hashlib.sha256(f.read(min(BLOCK, int(length) - o))).digest())
    return b"".join(out)


def block_proof(leaves, file_tree: bytes, m: int, height: int, piece: int, pos: int, span: int) -> bytes:
    """The `hashes` message for a base-layer-0 request of `span` leaf hashes (a
    power of two) at span number `pos` inside piece `piece` of a file: `leaves`
    is that piece's leaf layer (2^height rows, :func:`leaf_rows`), file_tree the
    tree of the file's m-row piece layer (:func:`build_tree` at `height`).  Rows,
    in order: the span's, the log2(2^height / span) uncles inside the piece,
    then the ceil(log2 m) uncles above it out of file_tree.  Equal to
    make_proof over the file's whole leaf layer at span number
    piece * (2^height / span) + pos."""
    rows = _rows(leaves)
    if len(rows) != 1 << height:
        raise ValueError("leaves must hold the piece's 2^height rows")
    if span < 1 or span & (span - 1) or span > len(rows):
        raise ValueError("span must be a power of two of at most 2^height")
    if not 0 <= piece < m or not 0 <= pos < len(rows) // span:
        raise ValueError("piece or pos outside the file")
    inside = make_proof(rows, 0, pos, span, height - (span.bit_length() - 1))
    above = proof_from_tree(file_tree, m, height, 0, piece, 1, (m - 1).bit_length())
    return inside + above[32:]
