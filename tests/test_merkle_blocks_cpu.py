"""CPU: the block checks' host side — merkle.leaf_rows, bad_blocks, bitmap_words
and block_proof against hand-written hashlib, vx_merkle_bitmap_words through
the library, the three prototypes as C99, and what the new entries refuse
before they touch a device.  No GPU, no compute calls."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

from conftest import ROOT

BLOCK = 16384
NEW = {"vx_merkle_bitmap_words", "vx_merkle_device_block_check", "vx_merkle_check_blocks"}


def _sha(a, b=b""):
    return hashlib.sha256(a + b).digest()


def _pad(height):
    h = bytes(32)
    for _ in range(height):
        h = _sha(h, h)
    return h


def _leaves(data, width):
    """Hand-written: the leaf rows of one piece of `width` slots."""
    out = []
    for b in range(width):
        out.append(_sha(data[b * BLOCK:(b + 1) * BLOCK]) if b * BLOCK < len(data) else bytes(32))
    return out


def _reduce(rows, height):
    """Root of a power-of-two-padded layer standing `height` above the leaves."""
    rows = list(rows)
    k = 0
    while len(rows) > 1:
        if len(rows) & 1:
            rows.append(_pad(height + k))
        rows = [_sha(rows[j], rows[j + 1]) for j in range(0, len(rows), 2)]
        k += 1
    return rows[0]


def walk(proof, pos, span, height):
    """A `hashes` message's rows reduced to the row its uncles reach."""
    rows = [proof[32 * k:32 * k + 32] for k in range(len(proof) // 32)]
    top = _reduce(rows[:span], height)
    for u in rows[span:]:
        top = _sha(u, top) if pos & 1 else _sha(top, u)
        pos >>= 1
    return top


# ---- header and exports -----------------------------------------------------------

def test_header_declares_the_new_entries_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "#if VX_ABI_VERSION != 3\n#error the block checks only add symbols: the ABI stays 3\n#endif\n"
                 "int main(void){\n"
                 "  uint64_t (*a)(uint32_t, uint32_t) = vx_merkle_bitmap_words;\n"
                 "  int (*b)(const void*, const uint64_t*, const uint32_t*, uint32_t, uint32_t, const void*, uint64_t*,"
                 " void*, void*) = vx_merkle_device_block_check;\n"
                 "  int (*d)(vx_ctx*, const uint8_t* const*, const uint32_t*, size_t, uint32_t, const uint8_t*,"
                 " uint64_t*, uint32_t*, uint8_t*) = vx_merkle_check_blocks;\n"
                 "  return !(a && b && d);\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_exports_and_abi(built):
    from test_abi import declared_symbols, dynamic_symbols
    from vortex_amd import _lib

    assert NEW <= declared_symbols() and NEW <= set(_lib.EXPORTS)
    assert NEW <= dynamic_symbols(_lib.LIB_PATH) and NEW <= dynamic_symbols(_lib.TUNING_PATH)
    assert _lib.lib().vx_abi_version() == 3 == _lib.ABI_VERSION


# ---- the Python models ---------------------------------------------------------------

@pytest.mark.parametrize("length,log2w", [(0, 0), (0, 3), (1, 0), (16383, 1), (16384, 0), (16385, 1),
                                          (3 * BLOCK + 77, 2), (3 * BLOCK + 77, 4), (8 * BLOCK, 3)])
def test_leaf_rows(length, log2w):
    from vortex_amd import merkle

    data = random.Random(length * 31 + log2w).randbytes(length)
    got = merkle.leaf_rows(data, log2w)
    assert got == b"".join(_leaves(data, 1 << log2w)) and len(got) == 32 << log2w
    assert merkle.leaf_rows(bytearray(data), log2w) == got
    # zero rows beyond the end, not the hash of an empty block
    used = (length + BLOCK - 1) // BLOCK
    assert got[32 * used:] == bytes(32 * ((1 << log2w) - used))
    assert _sha(b"") not in (got[32 * k:32 * k + 32] for k in range(used, 1 << log2w))


def test_leaf_rows_refuses():
    from vortex_amd import merkle

    with pytest.raises(ValueError):
        merkle.leaf_rows(bytes(BLOCK + 1), 0)
    with pytest.raises(ValueError):
        merkle.leaf_rows(b"", 18)
    with pytest.raises(ValueError):
        merkle.leaf_rows(b"", -1)


def test_bad_blocks():
    from vortex_amd import merkle

    rng = random.Random(0xB10C)
    good = rng.randbytes(5 * BLOCK + 100)  # 6 blocks in 8 slots, the last one short
    exp = _leaves(good, 8)
    assert merkle.bad_blocks(good, b"".join(exp)) == []
    assert merkle.bad_blocks(good, exp) == []  # a sequence of rows is a layer too
    for flips, want in (([0], [0]), ([BLOCK - 1], [0]), ([BLOCK], [1]), ([5 * BLOCK + 99], [5]),
                        ([0, 2 * BLOCK + 5, 5 * BLOCK], [0, 2, 5]), (list(range(0, len(good), BLOCK)), [0, 1, 2, 3, 4, 5])):
        data = bytearray(good)
        for o in flips:
            data[o] ^= 0x40
        assert merkle.bad_blocks(data, b"".join(exp)) == want
    # an expected row that is off, by its first or its last byte
    for b, byte in ((0, 0), (3, 31), (5, 0)):
        rows = [bytearray(r) for r in exp]
        rows[b][byte] ^= 1
        assert merkle.bad_blocks(good, b"".join(rows)) == [b]
    # garbage in the rows of slots beyond the piece's end never flags
    rows = exp[:6] + [rng.randbytes(32), rng.randbytes(32)]
    assert merkle.bad_blocks(good, b"".join(rows)) == []
    # a shorter piece against the same rows: only what it has is looked at
    assert merkle.bad_blocks(good[:2 * BLOCK], b"".join(exp)) == []
    assert merkle.bad_blocks(good[:2 * BLOCK - 1], b"".join(exp)) == [1]
    assert merkle.bad_blocks(b"", b"".join(exp)) == []
    with pytest.raises(ValueError):
        merkle.bad_blocks(bytes(2 * BLOCK + 1), b"".join(exp[:2]))


def test_bitmap_words_python():
    from vortex_amd import merkle

    for n in (0, 1, 3, 67):
        for lw in range(18):
            assert merkle.bitmap_words(n, lw) == n * (1 if lw < 6 else 1 << (lw - 6))
    assert merkle.bitmap_words(5, 18) == 0
    assert (merkle.bitmap_words(1, 5), merkle.bitmap_words(1, 6), merkle.bitmap_words(1, 7)) == (1, 1, 2)
    with pytest.raises(ValueError):
        merkle.bitmap_words(-1, 0)


def test_bitmap_words_library(built):
    from vortex_amd import _lib, merkle

    fn = _lib.lib().vx_merkle_bitmap_words
    for lw in range(18):
        for n in (0, 1, 3, 67, 0xFFFFFFFF):
            assert fn(n, lw) == merkle.bitmap_words(n, lw), (n, lw)
    assert fn(5, 18) == 0 and fn(0xFFFFFFFF, 17) == 0xFFFFFFFF * 2048  # no 32-bit wrap


# ---- block_proof ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def five_pieces():
    """A 5-piece file at 128 KiB pieces (W = 8), the last piece 2 blocks and 9 bytes."""
    from vortex_amd import merkle

    plen, height = 8 * BLOCK, 3
    body = random.Random(0xF11E).randbytes(4 * plen + 2 * BLOCK + 9)
    pieces = [body[o:o + plen] for o in range(0, len(body), plen)]
    leaves = [merkle.leaf_rows(p, height) for p in pieces]
    layer = [_reduce([lv[32 * k:32 * k + 32] for k in range(8)], 0) for lv in leaves]
    return body, pieces, leaves, layer, merkle.build_tree(layer, height), height


@pytest.mark.parametrize("span", [1, 2, 8])
@pytest.mark.parametrize("piece", [0, 4])
def test_block_proof_is_make_proof_over_the_whole_leaf_layer(built, five_pieces, span, piece):
    from vortex_amd import merkle

    body, pieces, leaves, layer, tree, height = five_pieces
    m, W = len(pieces), 1 << height
    # the file's leaf layer as BEP 52 has it: the blocks it has, nothing beyond
    whole = [_sha(body[o:o + BLOCK]) for o in range(0, len(body), BLOCK)]
    assert len(whole) == 4 * W + 3
    uncles = (height - (span.bit_length() - 1)) + 3  # inside the piece, then ceil(log2 5) above it
    root = _reduce(layer, height)
    assert tree[-32:] == root
    for pos in range(W // span):
        got = merkle.block_proof(leaves[piece], tree, m, height, piece, pos, span)
        file_pos = piece * (W // span) + pos
        assert got == merkle.make_proof(whole, 0, file_pos, span, uncles), (piece, pos, span)
        assert len(got) == 32 * (span + uncles)
        assert got[:32 * span] == leaves[piece][32 * span * pos:32 * span * (pos + 1)]
        assert walk(got, file_pos, span, 0) == root
        # ... and cut after the uncles inside the piece it ends at the piece's own row
        inside = got[:32 * (span + uncles - 3)]
        assert walk(inside, pos, span, 0) == layer[piece]


def test_block_proof_refuses(built, five_pieces):
    from vortex_amd import merkle

    _, pieces, leaves, _, tree, height = five_pieces
    m = len(pieces)
    for args in ((5, 0, 1), (-1, 0, 1), (0, 8, 1), (0, 0, 3), (0, 0, 16), (0, 1, 8), (0, 0, 0)):
        with pytest.raises(ValueError):
            merkle.block_proof(leaves[0], tree, m, height, *args)
    with pytest.raises(ValueError):
        merkle.block_proof(leaves[0][:-32], tree, m, height, 0, 0, 1)


# ---- what the entries refuse before a device is touched ---------------------------------------

def test_device_entry_validation_without_gpu(built):
    from vortex_amd import _lib

    L, E = _lib.lib(), _lib.VX_EINVAL
    p = ctypes.c_void_p
    fn = L.vx_merkle_device_block_check
    base, offs, lens, exp, bad, out = (p(0x10000), p(0x20000), p(0x30000), p(0x40000), p(0x50000), p(0x60000))
    assert fn(None, None, None, 0, 3, None, None, None, None) == 0  # n == 0 launches nothing
    assert fn(None, offs, lens, 4, 3, exp, bad, out, None) == E
    assert fn(base, None, lens, 4, 3, exp, bad, out, None) == E
    assert fn(base, offs, None, 4, 3, exp, bad, out, None) == E
    assert fn(base, offs, lens, 4, 3, exp, None, out, None) == E and b"together" in L.vx_last_error()
    assert fn(base, offs, lens, 4, 3, None, bad, out, None) == E and b"together" in L.vx_last_error()
    assert fn(base, offs, lens, 4, 3, None, None, None, None) == E
    assert fn(p(0x10008), offs, lens, 4, 3, exp, bad, out, None) == E
    assert fn(base, offs, lens, 4, 3, p(0x40008), bad, out, None) == E and b"aligned" in L.vx_last_error()
    assert fn(base, offs, lens, 4, 3, exp, p(0x50004), out, None) == E and b"aligned" in L.vx_last_error()
    assert fn(base, offs, lens, 4, 3, exp, bad, p(0x60008), None) == E
    assert fn(base, offs, lens, 4, 18, exp, bad, out, None) == E
    assert fn(base, offs, lens, 1 << 15, 17, exp, bad, out, None) == E and b"32 bits" in L.vx_last_error()


def test_context_entry_refuses_null_context(built):
    from vortex_amd import _lib

    L = _lib.lib()
    assert L.vx_merkle_check_blocks(None, None, None, 0, 16384, None, None, None, None) == _lib.VX_EINVAL
    assert b"NULL context" in L.vx_last_error()
