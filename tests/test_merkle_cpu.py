"""CPU: the BitTorrent v2 (BEP 52) merkle additions of the C ABI — header,
exports, argument validation, pad hashes — and merkle.file_pieces, checked
against hashlib and a pure-Python BEP 52 tree (no GPU, no compute calls)."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi import declared_symbols, dynamic_symbols

BLOCK = 16384
MERKLE = {"vx_merkle_device_uniform", "vx_merkle_device_ragged", "vx_merkle_device_root", "vx_merkle_pad_hash",
          "vx_merkle_verify_batch"}


def sha256(b):
    return hashlib.sha256(b).digest()


def pad(h):
    return bytes(32) if h == 0 else sha256(pad(h - 1) * 2)


def piece_root(data, log2w):
    """BEP 52: leaves over 16 KiB blocks (the last at its real length), zero
    hashes beyond the data, a binary tree over 2^log2w leaf slots."""
    nodes = [sha256(data[o:o + BLOCK]) if o < len(data) else bytes(32) for o in range(0, BLOCK << log2w, BLOCK)]
    while len(nodes) > 1:
        nodes = [sha256(nodes[k] + nodes[k + 1]) for k in range(0, len(nodes), 2)]
    return nodes[0]


def file_roots(data, piece_length):
    """BEP 52 from the file's side: `pieces root` of a file of at most
    piece_length bytes is the root over its blocks padded to a power of two;
    a longer file's `piece layers` are the roots of piece_length-wide subtrees."""
    if len(data) <= piece_length:
        blocks = -(-len(data) // BLOCK)
        w = 0
        while (1 << w) < blocks:
            w += 1
        return [piece_root(data, w)]
    full = (piece_length // BLOCK).bit_length() - 1
    return [piece_root(data[o:o + piece_length], full) for o in range(0, len(data), piece_length)]


def test_fips_vectors_of_the_yardstick():
    assert sha256(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert sha256(b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq").hex() == \
        "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"


def test_header_compiles_as_c99_with_merkle_names(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "int main(void){ unsigned char out[VX_SHA256_LEN];\n"
                 "  int (*f)(const void*, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t, void*, void*, const void*,"
                 " void*, void*) = vx_merkle_device_uniform;\n"
                 "  (void)f; return vx_merkle_pad_hash(0, out) + (VX_MERKLE_BLOCK != 16384) + (VX_ABI_VERSION != 3); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_merkle_exports(built):
    from vortex_amd import _lib

    decl = declared_symbols()
    assert MERKLE <= decl
    assert decl == set(_lib.EXPORTS)
    assert MERKLE <= dynamic_symbols(_lib.LIB_PATH) and MERKLE <= dynamic_symbols(_lib.TUNING_PATH)
    for L in (_lib.lib(), _lib.tuning()):
        assert L.vx_abi_version() == 3
        for name in MERKLE:
            assert getattr(L, name).argtypes is not None
    assert (_lib.VX_MERKLE_BLOCK, _lib.VX_SHA256_LEN) == (16384, 32)


def test_merkle_validation_without_gpu(built):
    from vortex_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p
    base, leaves = p(0x10000), p(0x20000)

    def uniform(d_base=base, stride=65536, length=65536, last=65536, n=4, lw=2, d_leaves=leaves):
        return L.vx_merkle_device_uniform(d_base, stride, length, last, n, lw, d_leaves, None, None, None, None)

    def einval(rc, word):
        assert rc == _lib.VX_EINVAL
        assert word in L.vx_last_error(), L.vx_last_error()

    einval(uniform(d_base=None), b"NULL")
    einval(uniform(d_leaves=None), b"NULL")
    einval(uniform(d_base=p(0x10008)), b"aligned")
    einval(uniform(stride=65536 + 8), b"stride")
    einval(uniform(stride=32768), b"stride < len")
    einval(uniform(last=0), b"last_len")
    einval(uniform(last=65537), b"last_len")
    einval(uniform(length=65536 + 16, stride=131072, last=1), b"log2_width")  # len > width * 16384
    einval(uniform(lw=18, length=16384, last=16384), b"log2_width > 17")
    einval(uniform(n=1 << 30, lw=2), b"32 bits")
    einval(uniform(n=1 << 15, lw=17, length=16384, last=16384), b"32 bits")
    assert uniform(n=0) == 0
    assert uniform(n=0, d_base=None, d_leaves=None) == 0  # n == 0 launches nothing, checks nothing

    def ragged(d_base=base, offs=p(0x30000), lens=p(0x40000), n=4, lw=2, d_leaves=leaves):
        return L.vx_merkle_device_ragged(d_base, offs, lens, None, n, lw, d_leaves, None, None, None, None)

    einval(ragged(d_base=None), b"NULL")
    einval(ragged(d_leaves=None), b"NULL")
    einval(ragged(offs=None), b"NULL")
    einval(ragged(lens=None), b"NULL")
    einval(ragged(d_base=p(0x10004)), b"aligned")
    einval(ragged(lw=18), b"log2_width > 17")
    einval(ragged(n=1 << 31, lw=1), b"32 bits")
    assert ragged(n=0) == 0

    einval(L.vx_merkle_device_root(None, 4, 0, p(0x1000), p(0x2000), None), b"NULL")
    einval(L.vx_merkle_device_root(p(0x1000), 4, 0, None, p(0x2000), None), b"NULL")
    einval(L.vx_merkle_device_root(p(0x1000), 4, 0, p(0x3000), None, None), b"NULL")
    einval(L.vx_merkle_device_root(p(0x1000), 4, 65, p(0x3000), p(0x2000), None), b"height")
    assert L.vx_merkle_device_root(None, 0, 0, None, None, None) == 0
    einval(L.vx_merkle_pad_hash(0, None), b"NULL")
    einval(L.vx_merkle_pad_hash(129, ctypes.create_string_buffer(32)), b"height")
    # the host batch refuses a NULL context before it looks at anything else
    einval(L.vx_merkle_verify_batch(None, None, None, None, 0, 16384, None, None, None), b"NULL context")


def test_pad_hash_matches_hashlib(built):
    from vortex_amd import _lib, merkle

    out = ctypes.create_string_buffer(32)
    for L in (_lib.lib(), _lib.tuning()):
        for h in range(18):
            assert L.vx_merkle_pad_hash(h, out) == 0
            assert out.raw == pad(h) == merkle.pad_hash(h), h
    # the pad hash of height h is the root of an empty piece of that height
    assert pad(4) == piece_root(b"", 4)


@pytest.mark.parametrize("piece_length", [16384, 262144, 2 << 20])
def test_file_pieces_against_python_tree(piece_length):
    from vortex_amd import merkle

    full = merkle.log2_width(piece_length)
    assert BLOCK << full == piece_length
    for flen in (1, 16384, 16385, piece_length, piece_length + 1, 3 * piece_length - 7):
        data = hashlib.shake_128(b"file %d" % flen).digest(flen)
        lens, log2w = merkle.file_pieces(flen, piece_length)
        assert sum(lens) == flen and len(lens) == len(log2w) == max(1, -(-flen // piece_length))
        assert all(0 < n <= BLOCK << w <= piece_length for n, w in zip(lens, log2w))
        if flen > piece_length:
            assert log2w == [full] * len(lens) and lens[:-1] == [piece_length] * (len(lens) - 1)
        else:  # the smallest tree that holds the file's blocks
            assert len(lens) == 1 and (log2w[0] == 0 or (BLOCK << (log2w[0] - 1)) < flen)
        got, o = [], 0
        for n, w in zip(lens, log2w):
            got.append(piece_root(data[o:o + n], w))
            o += n
        assert got == file_roots(data, piece_length)
    assert merkle.file_pieces(0, piece_length) == ([], [])
    with pytest.raises(ValueError):
        merkle.file_pieces(1, piece_length + 1)
    with pytest.raises(ValueError):
        merkle.log2_width(8192)


def test_device_lens_are_int32_and_a_2_gib_piece_is_refused():
    """device.py's layout check on host tensors (it runs wherever its tensors
    live): a full piece of a 2^17-slot tree is 2^31 bytes, which the C ABI's
    uint32 holds and an int32 tensor does not; its bits there are a negative
    length, refused by name.  2^31 - 1 bytes, the longest piece lens can hold,
    pass at width 17 and are too long for width 16."""
    import torch

    from vortex_amd import device as vdev

    class Sized:  # stands for a 2 GiB data tensor: the check reads its numel() only
        @staticmethod
        def numel():
            return 1 << 31

    offs = torch.tensor([0], dtype=torch.int64)
    with pytest.raises((RuntimeError, OverflowError)):
        torch.tensor([1 << 31], dtype=torch.int32)
    wrapped = torch.tensor([-1 << 31], dtype=torch.int32)  # the bits of uint32 2^31
    for who in ("merkle_ragged", "merkle_pieces", "merkle_block_check", "hybrid_pieces"):
        with pytest.raises(ValueError, match=who + ": negative offset or length .*2\\^31 bytes"):
            vdev._check_merkle_layout(Sized, offs, wrapped, None, 17, who)
    longest = torch.tensor([(1 << 31) - 1], dtype=torch.int32)
    vdev._check_merkle_layout(Sized, offs, longest, None, 17)
    vdev._check_merkle_layout(Sized, offs, longest, torch.tensor([17], dtype=torch.uint8), 17)
    with pytest.raises(ValueError, match="longer than its tree"):
        vdev._check_merkle_layout(Sized, offs, longest, None, 16)
    with pytest.raises(ValueError, match="longer than its tree"):
        vdev._check_merkle_layout(Sized, offs, longest, torch.tensor([16], dtype=torch.uint8), 17)
