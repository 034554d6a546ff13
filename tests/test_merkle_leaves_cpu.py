"""CPU: the leaf table of a v2 torrent (block checks from disk) — the layout of
vortex_amd/csrc/vx_merkle_leaves.hpp, run as a stand-alone program under
ASan+UBSan, against merkle.leaf_layout; the engine's rounds replayed with
hashlib in the kernels' place and a Python model of the leaf-check kernel's
lanes, waves and words, against the table and bitmap merkle.bad_blocks
predicts; the new C ABI entries (header, exports, validation).  No GPU."""
import ctypes
import hashlib
import json
import os
import random
import shutil
import subprocess

import pytest

import _layouts  # noqa: F401  (the golden layouts' home: tests/golden/vectors.json)
from conftest import ROOT
from test_abi import declared_symbols, dynamic_symbols

BLOCK = 16384
NEW = {"vx_merkle_leaf_rows", "vx_merkle_device_leaf_check", "vx_merkle_verify_files_blocks",
       "vx_merkle_verify_files_blocks_range", "vx_merkle_hash_files_leaves", "vx_merkle_hash_files_leaves_range"}


def _golden_layouts():
    """The reference's multi-file layouts, their byte counts taken as units of
    257 bytes: files of a few blocks with odd tails, empty files among them."""
    with open(os.path.join(ROOT, "tests", "golden", "vectors.json")) as f:
        entries = json.load(f)["file_store_layouts"]
    return {e["name"]: [f["len"] * 257 for f in e["files"]] for e in entries
            if len(e["files"]) > 1 and sum(f["len"] for f in e["files"]) < 20000}


SHAPES = dict(_golden_layouts())
SHAPES.update({
    "empty_files": [0, 0, 5, 0, BLOCK, 0],
    "one_byte": [1],
    "one_block": [BLOCK],
    "piece_plus_one_64k": [65536 + 1],
    "piece_plus_one_1m": [(1 << 20) + 1],
    "small_before_large": [1, 7, 20000, 3 * BLOCK, 1, BLOCK + 1] * 6 + [5 * 65536 + 100],
    "mixed": [0, 1, 16384, 16385, 3 * BLOCK, 65536, 65537, 2 * 65536 + 5, 0, 40000, 7, 5 * 65536, 1, 1, 30000],
})


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("lld") / "leaf_layout_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "leaf_layout_dump.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, flens, pl, first, count, bpr=0):
    out = subprocess.run([str(exe), str(pl), str(first), str(count)] + ([str(bpr)] if bpr else []),
                         input="\n".join(map(str, flens)) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = {"pieces": [], "rounds": []}
    for ln in out.stdout.split("\n"):
        if not ln:
            continue
        kind, *v = ln.split()
        v = [int(x) for x in v]
        if kind == "T":
            res["rows"] = v[0]
        elif kind == "L":
            res["ok"], res["base"], res["range_rows"] = v
        elif kind == "p":
            res["pieces"].append(tuple(v))
        elif kind == "R":
            res["rounds"].append({"data_blocks": v[0], "table": [], "nodes": []})
        elif kind == "t":
            res["rounds"][-1]["table"].append(v)
        elif kind == "n":
            res["rounds"][-1]["nodes"].append(v)
        elif kind == "W":
            res["window"] = v[0]
    return res


def _ranges(n):
    return [r for r in ((0, n), (0, 0), (n, 0), (1, 1), (1, n - 2), (n // 2, n - n // 2), (n - 1, 1), (2, 3))
            if r[0] + r[1] <= n and r[1] >= 0]


# ---- the model itself ---------------------------------------------------------

def test_leaf_layout_model():
    from vortex_amd import merkle

    pl = 65536
    flens = [0, 1, BLOCK, BLOCK + 1, pl, pl + 1, 0, 3 * pl - 5]
    first, blocks, rows = merkle.leaf_layout(flens, pl)
    assert rows == sum(-(-n // BLOCK) for n in flens) == 0 + 1 + 1 + 2 + 4 + 5 + 0 + 12
    #            f1  f2  f3  f4  f5: two pieces  f7: three pieces
    assert first == [0, 1, 2, 4, 8, 12, 13, 17, 21] and blocks == [1, 1, 2, 4, 4, 1, 4, 4, 4]
    # no padding row anywhere: the pieces' rows tile the table
    assert all(a + b == c for a, b, c in zip(first, blocks, first[1:] + [rows]))
    lens = merkle.torrent_pieces(flens, pl)[0]
    assert blocks == [-(-n // BLOCK) for n in lens]
    assert merkle.leaf_layout([], pl) == ([], [], 0) and merkle.leaf_layout([0, 0], pl) == ([], [], 0)
    with pytest.raises(ValueError):
        merkle.leaf_layout([1], pl + 1)


def test_file_leaf_table_is_the_pieces_leaf_rows(tmp_path):
    from vortex_amd import merkle

    rng = random.Random(7)
    flens = [0, 1, BLOCK, 65536 + 1, 40000]
    paths = []
    for k, n in enumerate(flens):
        paths.append(str(tmp_path / f"f{k}"))
        with open(paths[-1], "wb") as f:
            f.write(rng.randbytes(n))
    table = merkle.file_leaf_table(paths, flens, 65536)
    first, blocks, rows = merkle.leaf_layout(flens, 65536)
    assert len(table) == 32 * rows
    lens, log2w, findex, foff = merkle.torrent_pieces(flens, 65536)
    for i in range(len(lens)):
        with open(paths[findex[i]], "rb") as f:
            f.seek(foff[i])
            piece = f.read(lens[i])
        assert table[32 * first[i]:32 * (first[i] + blocks[i])] == merkle.leaf_rows(piece, log2w[i])[:32 * blocks[i]]


# ---- the header's layout against the model --------------------------------------

@pytest.mark.parametrize("pl", [16384, 65536, 1 << 20])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_layout_matches_the_model(dump, name, pl):
    from vortex_amd import merkle

    flens = SHAPES[name]
    first, blocks, rows = merkle.leaf_layout(flens, pl)
    n = len(first)
    for lo, count in _ranges(n):
        got = _run(dump, flens, pl, lo, count)
        assert got["rows"] == rows and got["ok"] == 1
        if count == 0:
            assert got["range_rows"] == 0 and got["pieces"] == []
            continue
        base = first[lo]
        assert got["base"] == base
        assert got["pieces"] == [(first[i] - base, blocks[i]) for i in range(lo, lo + count)]
        assert got["range_rows"] == first[lo + count - 1] + blocks[lo + count - 1] - base


def test_ranges_start_and_end_mid_file(dump):
    from vortex_amd import merkle

    flens = [3 * 65536 + 5, 7, 4 * 65536]
    first, blocks, _ = merkle.leaf_layout(flens, 65536)
    got = _run(dump, flens, 65536, 2, 5)  # piece 2 of file 0 to piece 1 of file 2
    assert got["base"] == 8 and got["pieces"] == [(0, 4), (4, 1), (5, 1), (6, 4), (10, 4)]
    assert got["range_rows"] == 14 and first[2] == 8 and first[6] + blocks[6] == 22


def test_a_range_of_2_to_the_32_rows_is_refused(dump):
    big = BLOCK << 32  # one file of exactly 2^32 blocks at 2 GiB pieces: 2^15 pieces
    assert _run(dump, [big], 1 << 31, 0, -1)["ok"] == 0
    got = _run(dump, [big], 1 << 31, 0, (1 << 15) - 1)  # all but the last piece: below 2^32
    assert got["ok"] == 1 and got["range_rows"] == (1 << 32) - (1 << 17)
    got = _run(dump, [big, 5], 1 << 31, (1 << 15) - 1, 2)  # a short range far into the table
    assert got["ok"] == 1 and got["base"] == (1 << 32) - (1 << 17) and got["pieces"] == [(0, 1 << 17), (1 << 17, 1)]


# ---- the rounds replayed: hashlib for the hash kernels, a model of the leaf check ----

def _leaf_check_model(window, row0, n, K, wpp, leaf_first, blocks, expected, bad, shadow, leaves_out):
    """merkle_leaf_check_kernel lane by lane, wave by wave: lane g = (k << K) +
    slot reads window row row0 + g; one ballot per 64 lanes; the word rules of
    vx_hash.h "The bitmap" with wpp words per piece."""
    rows = n << K
    for wave in range(0, rows, 64):
        mask = 0
        for lane in range(64):
            g = wave + lane
            if g >= rows:
                continue
            k, slot = g >> K, g & ((1 << K) - 1)
            live = slot < blocks[k]
            row = window[row0 + g]  # KeyError: the kernel would read a row no kernel wrote
            if leaves_out is not None and live:
                leaves_out[leaf_first[k] + slot] = row
            if expected is None:
                continue
            stored = expected[leaf_first[k] + slot] if live else bytes(32)
            shadow[row0 + g] = stored
            if live and stored != row:
                mask |= 1 << lane
        if expected is None:
            continue
        if K >= 6:
            k, slot = wave >> K, wave & ((1 << K) - 1)
            bad[k * wpp + (slot >> 6)] = mask
        else:
            for lane in range(0, min(64, rows - wave), 1 << K):
                bad[((wave + lane) >> K) * wpp] = (mask >> lane) & ((1 << (1 << K)) - 1)


def _root(rows, lw):
    rows = list(rows[:1 << lw])
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


def _replay(dump, flens, pl, lo, count, bpr, seed):
    from vortex_amd import merkle

    rng = random.Random(seed)
    lens, log2w, findex, foff = merkle.torrent_pieces(flens, pl)
    files = [rng.randbytes(n) for n in flens]
    pieces = [files[findex[i]][foff[i]:foff[i] + lens[i]] for i in range(len(lens))]
    first, blocks, _ = merkle.leaf_layout(flens, pl)
    got = _run(dump, flens, pl, lo, count, bpr)
    base = first[lo]
    rel_first, rel_blocks = [p[0] for p in got["pieces"]], [p[1] for p in got["pieces"]]
    table = [hashlib.sha256(p[o:o + BLOCK]).digest() for p in pieces[lo:lo + count] for o in range(0, len(p), BLOCK)]
    assert len(table) == got["range_rows"]
    # the stored table: every 5th row stale
    stored = list(table)
    stale = set(range(rng.randrange(5), len(stored), 5))
    for r in stale:
        stored[r] = hashlib.sha256(b"stale" + stored[r]).digest()
    wpp = max(1, pl // BLOCK // 64)
    bad = [0] * (count * wpp)  # cleared once, before the first round
    out = [None] * len(table)
    window, shadow = {}, {}
    blocks_in_order = [(i, k) for i in range(lo, lo + count) for k in range(blocks[i])]
    at = 0
    done = []
    layer_ok = {}
    widths = set()
    for r in got["rounds"]:
        for b, (row, ln) in enumerate(r["table"]):
            if b < r["data_blocks"]:
                i, k = blocks_in_order[at + b]
                window[row] = hashlib.sha256(pieces[i][k * BLOCK:k * BLOCK + ln]).digest()
            else:
                assert ln == 0
                window[row] = bytes(32)
        at += r["data_blocks"]
        for g_first, g_n, K, row0 in r["nodes"]:
            k0 = g_first - lo
            widths.add(K)
            assert max(1, (1 << K) // 64) <= wpp
            # slots past a narrow piece's own tree: never written by a hash kernel, the leaf check must not need them
            for g in range(g_n << K):
                window.setdefault(row0 + g, b"\xAA" * 32)
            _leaf_check_model(window, row0, g_n, K, wpp, rel_first[k0:k0 + g_n], rel_blocks[k0:k0 + g_n], stored,
                              _View(bad, k0 * wpp), shadow, out)
            for k in range(g_n):
                i = g_first + k
                rows_k = [shadow[row0 + (k << K) + s] for s in range(1 << K)]
                assert all(x == bytes(32) for x in rows_k[blocks[i]:])
                layer_ok[i] = _root(rows_k, log2w[i]) == _root(
                    [window[row0 + (k << K) + s] for s in range(1 << log2w[i])], log2w[i])
                done.append(i)
            for g in range(g_n << K):  # the rows are free for later groups
                del window[row0 + g]
    assert done == list(range(lo, lo + count))
    assert out == table, "copy-out is not the leaf table"
    for i in range(lo, lo + count):
        rows_i = b"".join(stored[first[i] - base:first[i] - base + blocks[i]])
        want = merkle.bad_blocks(pieces[i], rows_i)
        k = i - lo
        have = [64 * w + b for w in range(wpp) for b in range(64) if bad[k * wpp + w] >> b & 1]
        assert have == want, (i, have, want)
        assert layer_ok[i] == (not want)
    return widths


class _View:
    """bad + offset, as the launch passes it."""

    def __init__(self, words, off):
        self.words, self.off = words, off

    def __setitem__(self, k, v):
        self.words[self.off + k] = v


@pytest.mark.parametrize("pl", [16384, 65536, 1 << 20, 2 << 20])
def test_rounds_replayed_give_the_table_and_the_bitmap(dump, pl):
    """16-block rounds: they cut mid-piece, and the small files around a large
    one make groups narrower than the call (K < 6 under wpp = 2 at 2 MiB)."""
    flens = [1, 7, 20000, 3 * BLOCK, 0, BLOCK + 1] * 3 + [2 * pl + 5 * BLOCK + 9, pl + 1, 40000, pl]
    from vortex_amd import merkle

    n = len(merkle.torrent_pieces(flens, pl)[0])
    widths = _replay(dump, flens, pl, 0, n, 16, seed=pl)
    if pl >= 1 << 20:
        assert min(widths) < 6 <= max(widths), widths  # groups of mixed width did occur
    for lo, count in ((1, n - 2), (n // 2, n - n // 2), (n - 3, 2)):
        _replay(dump, flens, pl, lo, count, 16, seed=lo)


# ---- the C ABI ---------------------------------------------------------------

def test_header_declares_the_new_entries_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "int main(void){\n"
                 "  int64_t (*a)(const uint64_t*, size_t, uint32_t) = vx_merkle_leaf_rows;\n"
                 "  int (*b)(const void*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, const uint32_t*,"
                 " const void*, uint64_t*, void*, void*, void*) = vx_merkle_device_leaf_check;\n"
                 "  int64_t (*d)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, const uint8_t*, size_t,"
                 " const uint8_t*, uint64_t, uint8_t*, uint8_t*, uint64_t*, uint32_t*, uint32_t)"
                 " = vx_merkle_verify_files_blocks;\n"
                 "  int64_t (*e)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, const uint8_t*, size_t,"
                 " const uint8_t*, uint64_t, size_t, size_t, uint8_t*, uint8_t*, uint64_t*, uint32_t*, uint32_t)"
                 " = vx_merkle_verify_files_blocks_range;\n"
                 "  int64_t (*f)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, size_t, uint8_t*,"
                 " uint8_t*, uint8_t*, uint64_t, uint8_t*, uint64_t, uint32_t) = vx_merkle_hash_files_leaves;\n"
                 "  int64_t (*g)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, size_t, size_t, size_t,"
                 " uint8_t*, uint8_t*, uint8_t*, uint64_t, uint32_t) = vx_merkle_hash_files_leaves_range;\n"
                 "  (void)a; (void)b; (void)d; (void)e; (void)f; (void)g; return VX_ABI_VERSION != 3; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_new_entries_are_exported(built):
    from vortex_amd import _lib

    decl = declared_symbols()
    assert NEW <= decl and decl == set(_lib.EXPORTS)
    assert NEW <= dynamic_symbols(_lib.LIB_PATH) and NEW <= dynamic_symbols(_lib.TUNING_PATH)
    for L in (_lib.lib(), _lib.tuning()):
        assert L.vx_abi_version() == 3
        for name in NEW:
            assert getattr(L, name).argtypes is not None
    assert _lib.lib().vx_merkle_verify_files_blocks.restype is ctypes.c_int64


def test_leaf_rows_entry_matches_the_model(built):
    from vortex_amd import _lib, merkle

    L = _lib.lib()
    for name, flens in SHAPES.items():
        arr = (ctypes.c_uint64 * max(1, len(flens)))(*flens)
        for pl in (16384, 65536, 1 << 20):
            assert L.vx_merkle_leaf_rows(arr, len(flens), pl) == merkle.leaf_layout(flens, pl)[2], name
    one = (ctypes.c_uint64 * 1)(5)
    assert L.vx_merkle_leaf_rows(None, 0, 16384) == 0
    assert L.vx_merkle_leaf_rows(None, 1, 16384) == _lib.VX_EINVAL
    assert L.vx_merkle_leaf_rows(one, 1, 16384 * 3) == _lib.VX_EINVAL
    assert L.vx_merkle_leaf_rows(one, 1, 8192) == _lib.VX_EINVAL


def test_validation_without_gpu(built):
    """Everything the entries refuse before they touch a device."""
    from vortex_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p

    def einval(rc, word):
        assert rc == _lib.VX_EINVAL, rc
        assert word in L.vx_last_error(), L.vx_last_error()

    win, lf, bl, exp, bad, sh, out = (p(0x10000 * k) for k in range(1, 8))

    def leaf(window=win, row0=0, n=4, K=2, wpp=1, lf=lf, bl=bl, exp=exp, bad=bad, sh=sh, out=out):
        return L.vx_merkle_device_leaf_check(window, row0, n, K, wpp, lf, bl, exp, bad, sh, out, None)

    assert leaf(n=0, window=None, lf=None, bl=None, exp=None, bad=None, sh=None, out=None) == 0  # launches nothing
    einval(leaf(window=None), b"NULL")
    einval(leaf(lf=None), b"NULL")
    einval(leaf(bl=None), b"NULL")
    einval(leaf(exp=None), b"together")
    einval(leaf(bad=None), b"together")
    einval(leaf(exp=None, bad=None, sh=None, out=None), b"neither")
    einval(leaf(exp=None, bad=None, out=None), b"d_shadow_out needs")
    einval(leaf(K=18), b"log2_width > 17")
    einval(leaf(n=1 << 30, K=2), b"32 bits")
    einval(leaf(row0=0xFFFFFFFF), b"32 bits")
    einval(leaf(K=7, wpp=1), b"wpp")
    einval(leaf(wpp=0), b"wpp")
    einval(leaf(window=p(0x10008)), b"aligned")
    einval(leaf(exp=p(0x40008)), b"aligned")
    einval(leaf(sh=p(0x60004)), b"aligned")
    einval(leaf(out=p(0x70008)), b"aligned")
    einval(leaf(bad=p(0x50004)), b"aligned")
    einval(leaf(lf=p(0x20002)), b"aligned")
    einval(leaf(out=exp), b"one buffer")

    # the files calls, with a context pointer the entry must not reach
    paths = (ctypes.c_char_p * 2)(b"/nonexistent/a", b"/nonexistent/b")
    flens = (ctypes.c_uint64 * 2)(100000, 5)  # at 64 KiB: 2 + 1 pieces, 7 + 1 leaf rows
    roots = ctypes.create_string_buffer(32 * 3)
    leaves = ctypes.create_string_buffer(32 * 8)
    m, ok = ctypes.create_string_buffer(3), ctypes.create_string_buffer(3)
    words = (ctypes.c_uint64 * 3)()
    counts = (ctypes.c_uint32 * 3)()
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, p)

    def blocks(ctx=ctx, roots=roots, leaves=leaves, rows=8, m=m, ok=ok, words=words, counts=counts, n=3, pl=65536):
        return L.vx_merkle_verify_files_blocks(ctx, paths, flens, 2, pl, roots, n, leaves, rows, m, ok, words,
                                               counts, 0)

    def hashed(ctx=ctx, leaves=leaves, rows=8, n=3, out=roots):
        return L.vx_merkle_hash_files_leaves(ctx, paths, flens, 2, 65536, n, out, None, None, 0, leaves, rows, 0)

    einval(blocks(ctx=None), b"NULL context")
    einval(blocks(roots=None), b"NULL")
    einval(blocks(leaves=None), b"NULL")
    einval(blocks(m=None), b"NULL")
    einval(blocks(words=None), b"NULL")
    einval(blocks(n=2), b"n_pieces")
    einval(blocks(pl=3 * 16384), b"power of two")
    einval(L.vx_merkle_verify_files_blocks_range(ctx, paths, flens, 2, 65536, roots, 3, leaves, 8, 2, 2, m, ok, words,
                                                 counts, 0), b"range")
    einval(hashed(ctx=None), b"NULL context")
    einval(hashed(out=None), b"NULL rows_out")
    einval(hashed(leaves=None), b"NULL")
    einval(hashed(n=4), b"n_pieces")
