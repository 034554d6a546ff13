"""CPU: the v2 re-verify from disk — merkle.torrent_pieces, the four new C ABI
entries (header, exports, argument validation) and the round packer
(vortex_amd/csrc/vx_merkle_rounds.hpp), run as a stand-alone program under
ASan+UBSan and checked against a Python model of BEP 52's piece layout; then
its rounds read from real files by the reader pool, also stand-alone under
ASan+UBSan.  No GPU, no compute calls."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_abi import declared_symbols, dynamic_symbols

BLOCK = 16384
NEW = {"vx_merkle_device_blocks", "vx_merkle_device_nodes", "vx_merkle_verify_files", "vx_merkle_verify_files_range"}


@pytest.mark.parametrize("piece_length", [16384, 65536, 1 << 20])
def test_torrent_pieces_is_file_pieces_file_by_file(piece_length):
    from vortex_amd import merkle

    pl = piece_length
    flens = [0, 1, 16384, 16385, pl, pl + 1, 3 * pl, 0, 1]
    lens, log2w, findex, foff = merkle.torrent_pieces(flens, pl)
    want_l, want_w, want_f, want_o = [], [], [], []
    for f, n in enumerate(flens):
        fl, fw = merkle.file_pieces(n, pl)
        want_l += fl
        want_w += fw
        want_f += [f] * len(fl)
        want_o += [k * pl for k in range(len(fl))]
    assert (lens, log2w, findex, foff) == (want_l, want_w, want_f, want_o)
    assert len(lens) == sum(-(-n // pl) for n in flens) and sum(lens) == sum(flens)
    # no piece spans files, and the pieces of a file tile it
    for f, n in enumerate(flens):
        mine = [(o, ln) for o, ln, g in zip(foff, lens, findex) if g == f]
        assert sum(ln for _, ln in mine) == n
        assert all(o == k * pl for k, (o, _) in enumerate(mine))
    assert merkle.torrent_pieces([], pl) == ([], [], [], [])
    with pytest.raises(ValueError):
        merkle.torrent_pieces([1], pl + 1)


def test_header_declares_the_new_entries_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "int main(void){\n"
                 "  int (*b)(const void*, const uint32_t*, const uint32_t*, uint32_t, void*, void*)"
                 " = vx_merkle_device_blocks;\n"
                 "  int (*n)(const void*, const uint8_t*, uint32_t, uint32_t, void*, const void*, void*, void*)"
                 " = vx_merkle_device_nodes;\n"
                 "  int64_t (*f)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, const uint8_t*,"
                 " size_t, uint8_t*, uint32_t) = vx_merkle_verify_files;\n"
                 "  int64_t (*r)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, const uint8_t*,"
                 " size_t, size_t, size_t, uint8_t*, uint32_t) = vx_merkle_verify_files_range;\n"
                 "  (void)b; (void)n; (void)f; (void)r; return VX_ABI_VERSION != 3; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_new_entries_are_exported(built):
    from vortex_amd import _lib

    decl = declared_symbols()
    assert NEW <= decl and NEW <= set(_lib.EXPORTS)
    assert decl == set(_lib.EXPORTS)
    assert NEW <= dynamic_symbols(_lib.LIB_PATH) and NEW <= dynamic_symbols(_lib.TUNING_PATH)
    for L in (_lib.lib(), _lib.tuning()):
        assert L.vx_abi_version() == 3
        for name in NEW:
            assert getattr(L, name).argtypes is not None
    assert _lib.lib().vx_merkle_verify_files.restype is ctypes.c_int64


def test_validation_without_gpu(built):
    """Everything the entries refuse before they touch a device."""
    from vortex_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p

    def einval(rc, word):
        assert rc == _lib.VX_EINVAL, rc
        assert word in L.vx_last_error(), L.vx_last_error()

    stage, rows, lens, leaves = p(0x10000), p(0x20000), p(0x30000), p(0x40000)
    einval(L.vx_merkle_device_blocks(None, rows, lens, 4, leaves, None), b"NULL")
    einval(L.vx_merkle_device_blocks(stage, None, lens, 4, leaves, None), b"NULL")
    einval(L.vx_merkle_device_blocks(stage, rows, None, 4, leaves, None), b"NULL")
    einval(L.vx_merkle_device_blocks(stage, rows, lens, 4, None, None), b"NULL")
    einval(L.vx_merkle_device_blocks(p(0x10008), rows, lens, 4, leaves, None), b"aligned")
    einval(L.vx_merkle_device_blocks(stage, p(0x20002), lens, 4, leaves, None), b"aligned")
    assert L.vx_merkle_device_blocks(None, None, None, 0, None, None) == 0  # n == 0 launches nothing
    einval(L.vx_merkle_device_nodes(None, None, 4, 2, p(0x50000), None, None, None), b"NULL")
    einval(L.vx_merkle_device_nodes(p(0x40008), None, 4, 2, p(0x50000), None, None, None), b"aligned")
    einval(L.vx_merkle_device_nodes(leaves, None, 4, 18, p(0x50000), None, None, None), b"log2_width > 17")
    einval(L.vx_merkle_device_nodes(leaves, None, 1 << 30, 2, p(0x50000), None, None, None), b"32 bits")
    einval(L.vx_merkle_device_nodes(leaves, None, 4, 2, p(0x50008), None, None, None), b"aligned")
    assert L.vx_merkle_device_nodes(None, None, 0, 0, None, None, None, None) == 0

    # the host entry: a NULL context first, then the tables, then the geometry.
    # No context can be made without a device, so the rest is checked with a
    # context pointer the entry must not reach: every case below fails on its
    # arguments alone.
    paths = (ctypes.c_char_p * 2)(b"/nonexistent/a", b"/nonexistent/b")
    flens = (ctypes.c_uint64 * 2)(100000, 5)
    exp = ctypes.create_string_buffer(32 * 8)
    out = ctypes.create_string_buffer(8)

    def files(ctx=None, paths=paths, flens=flens, nfiles=2, pl=65536, exp=exp, n=3, out=out):
        return L.vx_merkle_verify_files(ctx, paths, flens, nfiles, pl, exp, n, out, 0)

    def frange(first, count, ctx=None, n=3, pl=65536):
        return L.vx_merkle_verify_files_range(ctx, paths, flens, 2, pl, exp, n, first, count, out, 0)

    einval(files(), b"NULL context")
    einval(frange(0, 3), b"NULL context")
    # a context that is never dereferenced before the argument checks fail
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, p)
    einval(files(ctx, paths=None), b"NULL")
    einval(files(ctx, flens=None), b"NULL")
    einval(files(ctx, exp=None), b"NULL")
    einval(files(ctx, out=None), b"NULL")
    einval(files(ctx, pl=65536 + 16384), b"power of two")
    einval(files(ctx, pl=3 * 16384), b"power of two")
    einval(files(ctx, pl=8192), b">= 16384")
    einval(files(ctx, pl=0), b">= 16384")
    einval(files(ctx, n=2), b"n_pieces")   # 100000 bytes at 64 KiB: 2 pieces, and 5 bytes: 1
    einval(files(ctx, n=4), b"n_pieces")
    einval(files(ctx, pl=16384, n=3), b"n_pieces")  # 7 + 1 at 16 KiB
    einval(frange(4, 0, ctx), b"range")
    einval(frange(2, 2, ctx), b"range")
    einval(frange(0, 3, ctx, n=5), b"n_pieces")


# ---- the round packer ------------------------------------------------------

def _dump_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("mrd") / "merkle_rounds_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "merkle_rounds_dump.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _dump_exe(tmp_path_factory)


def _run(exe, flens, pl, first, count, bpr, window=0, entries=0, max_run=256, quiet=0):
    out = subprocess.run([str(exe), str(pl), str(first), str(count), str(bpr), str(window), str(entries),
                          str(max_run), str(quiet)], input="\n".join(map(str, flens)) + "\n", capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.rstrip("\n").split("\n")
    summary = json.loads(lines[-1])
    rounds = []
    for ln in lines[:-1]:
        kind, *v = ln.split()
        v = [int(x) for x in v]
        if kind == "R":
            rounds.append({"data_blocks": v[0], "bytes": v[1], "file_bytes": v[2], "reads": [], "table": [],
                           "nodes": []})
        elif kind == "r":
            rounds[-1]["reads"].append(v)
        elif kind == "t":
            rounds[-1]["table"].append(v)
        else:
            rounds[-1]["nodes"].append(v)
    return rounds, summary


def _check(exe, flens, pl, bpr, first=0, count=None, window=0, entries=0, max_run=256):
    """Rebuild the rounds' content from a Python model of the layout and check
    the packer's output against it."""
    from vortex_amd import merkle

    lens, log2w, findex, foff = merkle.torrent_pieces(flens, pl)
    n = len(lens)
    count = n - first if count is None else count
    rounds, summary = _run(exe, flens, pl, first, count, bpr, window, entries, max_run)
    R, cap = summary["window_rows"], summary["max_entries"]
    assert summary["pieces"] == n and R & (R - 1) == 0
    # the model: every block of every piece in range, in order
    want = [(i, k, findex[i], foff[i] + k * BLOCK, min(BLOCK, lens[i] - k * BLOCK))
            for i in range(first, first + count) for k in range(-(-lens[i] // BLOCK))]
    absent_want = sum((1 << log2w[i]) - -(-lens[i] // BLOCK) for i in range(first, first + count))
    at = 0          # next model block
    held = {}       # ring row -> (piece, slot, len): written, its piece not reduced yet
    launched = set()
    absent_seen = 0
    for r in rounds:
        nd = r["data_blocks"]
        assert 0 < len(r["table"]) <= cap and nd <= bpr
        # the reads tile stage blocks [0, nd) with 16 KiB-aligned runs that start at a block boundary of a file
        per_block = []
        for file, off, ln, sb, piece in r["reads"]:
            assert sb == len(per_block) and off % BLOCK == 0 and 0 < ln <= max_run * BLOCK
            assert off + ln <= flens[file]
            assert ln % BLOCK == 0 or off + ln == flens[file]  # only a file's last block is short
            assert piece == want[at + sb][0]                    # the piece of the run's first block
            per_block += [(file, off + o, min(BLOCK, ln - o)) for o in range(0, ln, BLOCK)]
        assert len(per_block) == nd
        assert r["bytes"] == (nd - 1) * BLOCK + per_block[-1][2] if nd else r["bytes"] == 0
        assert r["file_bytes"] == sum(b[2] for b in per_block)
        written = set()
        for b, (row, ln) in enumerate(r["table"]):
            assert 0 <= row < R
            assert row not in written and row not in held, "a row written twice while it was still needed"
            written.add(row)
            if b < nd:
                piece, k, file, off, want_len = want[at + b]
                assert per_block[b] == (file, off, want_len) and ln == want_len > 0
                held[row] = (piece, k, ln)
            else:
                assert ln == 0  # an absent slot: which one is settled by the node launch below
                held[row] = None
                absent_seen += 1
        at += nd
        for g_first, g_n, K, row0 in r["nodes"]:
            assert g_n > 0 and row0 + (g_n << K) <= R and row0 % (1 << K) == 0
            for k in range(g_n):
                piece = g_first + k
                assert first <= piece < first + count and piece not in launched and log2w[piece] <= K
                launched.add(piece)
                nb = -(-lens[piece] // BLOCK)
                for s in range(1 << log2w[piece]):
                    got = held.pop(row0 + (k << K) + s)  # KeyError: a slot of the tree was never written
                    assert got == ((piece, s, min(BLOCK, lens[piece] - s * BLOCK)) if s < nb else None)
    assert at == len(want), "blocks missing"
    assert launched == set(range(first, first + count)), "a piece was never reduced"
    assert not held, "rows written that no node launch reads"
    assert absent_seen == absent_want
    assert summary["blocks"] == len(want) and summary["rounds"] == len(rounds)
    return rounds, summary


@pytest.mark.parametrize("bpr", [1, 3, 16])
def test_packer_shapes(dump, bpr):
    # 1,000 files of 1 byte: a wave of tails, one piece each
    for pl in (16384, 65536):
        rounds, s = _check(dump, [1] * 1000, pl, bpr)
        assert s["rounds"] == -(-1000 // bpr) and s["entries"] == 1000
        assert all(len(r["reads"]) == r["data_blocks"] for r in rounds)  # a file's last block ends its run
    # one file of 5 blocks at 128 KiB pieces: width 8, three absent slots
    rounds, s = _check(dump, [5 * BLOCK], 131072, bpr)
    assert s["entries"] == 8 and s["launches"] == 1 and rounds[-1]["nodes"][0][2] == 3
    _check(dump, [5 * BLOCK - 100], 131072, bpr)
    # pl + 1 bytes: the second piece is one 1-byte block and width - 1 absent slots
    for pl in (65536, 1 << 20):
        rounds, s = _check(dump, [pl + 1], pl, bpr)
        w = pl // BLOCK
        assert s["entries"] == 2 * w and all(t[1] == 0 for t in rounds[-1]["table"][-(w - 1):])
        assert sum(t[1] for r in rounds for t in r["table"]) == pl + 1
    # a piece of 64 blocks across rounds
    rounds, s = _check(dump, [1 << 20, 3 << 20], 1 << 20, bpr)
    assert s["rounds"] == -(-256 // bpr)


def test_packer_piece_of_64_blocks_in_rounds_of_16(dump):
    rounds, s = _check(dump, [1 << 20], 1 << 20, 16)
    assert [r["data_blocks"] for r in rounds] == [16, 16, 16, 16]
    assert [len(r["nodes"]) for r in rounds] == [0, 0, 0, 1] and rounds[-1]["nodes"][0][1:3] == [1, 6]
    assert all(len(r["reads"]) == 1 for r in rounds)  # one pread per run
    rounds, _ = _check(dump, [1 << 20], 1 << 20, 16, max_run=4)
    assert all(len(r["reads"]) == 4 for r in rounds)


MIXED = [0, 1, 16384, 16385, 3 * BLOCK, 65536, 65537, 2 * 65536 + 5, 0, 40000, 7, 5 * 65536, 1, 1, 30000]


@pytest.mark.parametrize("pl", [16384, 65536, 1 << 20])
@pytest.mark.parametrize("bpr", [1, 3, 16])
def test_packer_mixed_torrent_and_ranges(dump, pl, bpr):
    from vortex_amd import merkle

    n = len(merkle.torrent_pieces(MIXED, pl)[0])
    _check(dump, MIXED, pl, bpr)
    for first, count in ((0, 0), (1, 1), (2, n - 3), (n // 2, n - n // 2), (n - 1, 1), (n, 0), (3, 4)):
        if first + count <= n:
            rounds, _ = _check(dump, MIXED, pl, bpr, first, count)
            assert bool(rounds) == bool(count)


def test_packer_small_window_and_small_tables(dump):
    """A window of 64 rows cuts rounds at the window; a table of blocks + width
    entries cuts rounds at the table; groups of 80 rows (a 10-block file and
    four 1-byte files: the density rule stops there) wrap a window of 1,024
    rows between two pieces and become two launches."""
    flens = [1] * 50 + [65537] * 5 + [3 * BLOCK] * 20 + [4 * 65536 + 1] + [1] * 70
    for bpr in (1, 3, 16):
        _check(dump, flens, 65536, bpr, window=64)
        rounds, _ = _check(dump, ([10 * BLOCK] + [1] * 4) * 30, 1 << 20, bpr, window=1024)
        assert any(n[3] == 0 and k > 0 and r["nodes"][k - 1][0] + r["nodes"][k - 1][1] == n[0]
                   for r in rounds for k, n in enumerate(r["nodes"])), "no group wrapped"
        rounds, _ = _check(dump, flens, 65536, bpr, window=64, entries=bpr + 4)
        if bpr == 16:  # five 3-block files fill the table (15 blocks + 5 absent slots) before the stage
            assert any(r["data_blocks"] < bpr for r in rounds[:-1]), "no round was cut early"
    _check(dump, [16385] * 40, 1 << 20, 16, window=1024, entries=16 + 64)


LARGE = [  # (piece_length, file_lengths, blocks_per_round): trees of 2^11, 2^13 and 2^17 (the widest) leaf slots
    (32 << 20, lambda pl: [pl + 1, 5, 2 * pl + BLOCK + 7], 256),
    (32 << 20, lambda pl: [pl + 1], 16),
    (1 << 27, lambda pl: [2 * pl + 77, 9], 1024),
    (1 << 31, lambda pl: [pl + 1], 4096),
    (1 << 31, lambda pl: [3 * BLOCK + 5, pl + BLOCK, 1], 16384),
]


@pytest.mark.parametrize("pl,flens,bpr", LARGE, ids=[f"{pl >> 20}MiB-{k}" for k, (pl, _, _) in enumerate(LARGE)])
def test_packer_large_piece_lengths(dump, pl, flens, bpr):
    """Pieces of 32 MiB, 128 MiB and 2 GiB (VX_MERKLE_MAX_LOG2_WIDTH): a piece
    takes many rounds, and a one-byte piece behind a full one leaves up to
    2^17 - 1 absent slots."""
    from vortex_amd import merkle

    flens = flens(pl)
    rounds, s = _check(dump, flens, pl, bpr)
    assert s["blocks"] == sum(-(-n // BLOCK) for n in flens)
    assert s["entries"] == sum(1 << w for w in merkle.torrent_pieces(flens, pl)[1])
    assert max(n[2] for r in rounds for n in r["nodes"]) == merkle.log2_width(pl)


def test_packer_100k_files(dump):
    """10^5 files: the packer walks pieces, not files per piece; its time is
    bounded as the v1 segment walk's is (tests/test_native_cpu.py), here under
    ASan+UBSan at -O1."""
    import numpy as np

    rng = np.random.default_rng(7)
    flens = rng.integers(0, 60000, 100000).tolist()
    _, s = _run(dump, flens, 16384, 0, -1, 4096, quiet=1)
    blocks = sum(-(-n // BLOCK) for n in flens)
    assert s["blocks"] == blocks == s["pieces"] and s["rounds"] == -(-blocks // 4096)
    assert s["build_ms"] < 2000, s
    _, s = _run(dump, flens, 1 << 20, 0, -1, 4096, quiet=1)
    assert s["blocks"] == blocks and s["pieces"] == sum(1 for n in flens if n)
    assert s["entries"] == sum(1 << (-(-n // BLOCK) - 1).bit_length() for n in flens if n)
    assert s["build_ms"] < 2000, s


# ---- the read side: rounds read by the reader pool in blocks mode ------------

@pytest.mark.parametrize("direct", [0, 1])
def test_rounds_read_by_the_reader_pool(tmp_path, direct):
    """tests/native/merkle_readers_check.cpp under ASan + UBSan: every round's
    runs land where the tables say (each block compared with the file's
    pattern), and a missing, short or truncated-at-a-block file marks exactly
    the pieces that lack bytes; a file longer than declared marks none."""
    from vortex_amd import merkle

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "merkle_readers_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "merkle_readers_check.cpp"), "-o", str(exe), "-lpthread"],
                   check=True)
    pl = 65536
    #        declared, actual (-1: missing)
    files = [(200000, 200000), (1, 1), (65537, -1), (100000, BLOCK), (0, 0), (3 * BLOCK, 3 * BLOCK + 99),
             (3 * 65536 + 5, 65536 + 20000), (1 << 20 | 4097, 1 << 20 | 4097), (40000, 39999), (7, 7)]
    lens, _, findex, foff = merkle.torrent_pieces([d for d, _ in files], pl)
    want_bad = [i for i in range(len(lens)) if foff[i] + lens[i] > max(files[findex[i]][1], 0)]
    assert want_bad  # pieces 5-6 (missing), 7-8 (cut to one block), part of file 6, the last piece of file 8
    data = tmp_path / "data"
    data.mkdir()
    for bpr, threads in ((1, 1), (3, 4), (16, 4), (64, 2)):
        out = subprocess.run([str(exe), str(data), str(pl), str(bpr), str(threads), str(direct)],
                             input="".join(f"{d} {a}\n" for d, a in files), capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        got = json.loads(out.stdout.strip().splitlines()[-1])
        assert got["pieces"] == len(lens) and got["mismatches"] == 0, got
        assert got["bad"] == want_bad, (bpr, got)
