"""CPU: the layer trees and the hash calls — the planner of
vx_merkle_device_trees replayed in Python with hashlib in the kernel's place
against merkle.build_tree and run as a stand-alone program under ASan+UBSan
(vortex_amd/csrc/vx_merkle_tree.hpp), vx_merkle_tree_proof against
merkle.make_proof and a plain hashlib walk, vx_merkle_tree_layout against
merkle.tree_layout, and what the new entries refuse before they touch a
device.  No GPU, no compute calls."""
import ctypes
import hashlib
import json
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_abi import declared_symbols, dynamic_symbols

NEW = {"vx_merkle_tree_rows", "vx_merkle_tree_plan", "vx_merkle_device_trees", "vx_merkle_build_trees",
       "vx_merkle_tree_proof", "vx_merkle_tree_layout", "vx_hash_files", "vx_hash_files_range",
       "vx_merkle_hash_files", "vx_merkle_hash_files_range", "vx_hybrid_hash_files", "vx_hybrid_hash_files_range"}
# one, two and three passes, and every edge of a tile
COUNTS = [1, 2, 3, 5, 511, 512, 513, 1023, 1024, 1025, 262144, 262145]


def _sha(a, b):
    return hashlib.sha256(a + b).digest()


def _pad(height):
    h = bytes(32)
    for _ in range(height):
        h = _sha(h, h)
    return h


# ---- header, layouts, exports ---------------------------------------------------

def test_header_declares_the_new_entries_as_c99(tmp_path):
    files = "vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, size_t"
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "int main(void){\n"
                 "  uint64_t (*a)(uint64_t) = vx_merkle_tree_rows;\n"
                 "  int (*b)(const uint32_t*, uint32_t, struct vx_merkle_tree_plan*, vx_merkle_tree_tile*, size_t,"
                 " uint64_t*) = vx_merkle_tree_plan;\n"
                 "  int (*d)(const void*, const struct vx_merkle_tree_plan*, const vx_merkle_tree_tile*, uint32_t,"
                 " void*, void*) = vx_merkle_device_trees;\n"
                 "  int (*e)(vx_ctx*, const uint8_t*, const uint32_t*, uint32_t, uint32_t, uint8_t*, uint8_t*)"
                 " = vx_merkle_build_trees;\n"
                 "  int (*f)(const uint8_t*, uint32_t, uint32_t, uint32_t, uint64_t, uint32_t, uint32_t, uint8_t*)"
                 " = vx_merkle_tree_proof;\n"
                 "  int64_t (*g)(const uint64_t*, size_t, uint32_t, uint32_t*, uint64_t*) = vx_merkle_tree_layout;\n"
                 f"  int64_t (*h)({files}, uint8_t*, uint8_t*, uint32_t) = vx_hash_files;\n"
                 f"  int64_t (*i)({files}, size_t, size_t, uint8_t*, uint8_t*, uint32_t) = vx_hash_files_range;\n"
                 f"  int64_t (*j)({files}, uint8_t*, uint8_t*, uint8_t*, uint64_t, uint32_t) = vx_merkle_hash_files;\n"
                 f"  int64_t (*k)({files}, size_t, size_t, uint8_t*, uint8_t*, uint32_t) = vx_merkle_hash_files_range;\n"
                 f"  int64_t (*l)({files}, uint8_t*, uint8_t*, uint8_t*, uint8_t*, uint64_t, uint32_t)"
                 " = vx_hybrid_hash_files;\n"
                 f"  int64_t (*m)({files}, size_t, size_t, uint8_t*, uint8_t*, uint8_t*, uint32_t)"
                 " = vx_hybrid_hash_files_range;\n"
                 "  (void)a; (void)b; (void)d; (void)e; (void)f; (void)g; (void)h; (void)i; (void)j; (void)k; (void)l;"
                 " (void)m;\n"
                 "  return VX_ABI_VERSION != 3; }\n")
    for compiler, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        if shutil.which(compiler) is None:
            continue
        src = c if compiler == "gcc" else tmp_path / "t.cpp"
        if src != c:
            src.write_text(c.read_text())
        subprocess.run([compiler, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], check=True)


@pytest.mark.parametrize("struct,ctype,size", [
    ("vx_merkle_tree_tile", "vx_merkle_tree_tile", 16),
    ("vx_merkle_tree_plan", "struct vx_merkle_tree_plan", 48)])
def test_struct_layouts(tmp_path, struct, ctype, size):
    """The two structs as ctypes have the C layout: size, a multiple of 16
    bytes, and every field's offset; C says so, compiled here."""
    from vortex_amd import _lib

    cls = getattr(_lib, struct)
    names = [n for n, _ in cls._fields_]
    c = tmp_path / "o.c"
    body = ", ".join(f"offsetof({ctype}, {f})" for f in names)
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vx_hash.h"\nint main(void){size_t o[] = {'
                 + body + '}; printf("%zu", sizeof(' + ctype + ')); for (size_t i = 0; i < sizeof(o) / sizeof(o[0]); '
                 '++i) printf(" %zu", o[i]); printf("\\n"); return 0;}\n')
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in names]
    assert got[0] == size and size % 16 == 0


def test_new_entries_are_exported(built):
    from vortex_amd import _lib

    decl = declared_symbols()
    assert NEW <= decl and NEW <= set(_lib.EXPORTS)
    assert NEW <= dynamic_symbols(_lib.LIB_PATH) and NEW <= dynamic_symbols(_lib.TUNING_PATH)
    for L in (_lib.lib(), _lib.tuning()):
        assert L.vx_abi_version() == 3
        for name in NEW:
            assert getattr(L, name).argtypes is not None


# ---- the planner, replayed -------------------------------------------------------

def _plan(counts):
    from vortex_amd import _lib

    L = _lib.lib()
    carr = (ctypes.c_uint32 * len(counts))(*counts)
    plan = _lib.vx_merkle_tree_plan()
    off0 = (ctypes.c_uint64 * (len(counts) + 1))()
    assert L.vx_merkle_tree_plan(carr, len(counts), ctypes.byref(plan), None, 0, off0) == 0
    tiles = (_lib.vx_merkle_tree_tile * plan.n_tiles)()
    off = (ctypes.c_uint64 * (len(counts) + 1))()
    assert L.vx_merkle_tree_plan(carr, len(counts), ctypes.byref(plan), tiles, plan.n_tiles, off) == 0
    assert list(off) == list(off0) and plan._pad == 0
    summary = {"n_layers": plan.n_layers, "passes": plan.passes, "rows": plan.rows, "tree_rows": plan.tree_rows,
               "n_tiles": plan.n_tiles, "pass_tiles": list(plan.pass_tiles)}
    at, out = 0, []
    for p in range(plan.passes):
        for _ in range(plan.pass_tiles[p]):
            t = tiles[at]
            out.append((p, t.src_row, t.dst_row, t.level_rows, t.tile))
            at += 1
    return summary, out, list(off)


@pytest.fixture(scope="module")
def layer_rows():
    """The input of every replay: random rows, as many as the counts need (built once)."""
    rng = random.Random(0x7AEE5)
    blob = rng.randbytes(32 * sum(COUNTS))
    return [blob[k:k + 32] for k in range(0, len(blob), 32)]


def replay(summary, tiles, rows, height):
    """Execute the tiles pass by pass with hashlib in merkle_tree_kernel's
    place: a tile loads its rows (the rest of the 512 are the pass's pad hash),
    stores them as level 0 in pass 0, and after each level of the reduction
    stores the rows of that level that exist.  Returns the tree buffer; checks
    on the way that no tile reads a row written in its own pass and that every
    tree row is written exactly once."""
    assert summary["rows"] == len(rows) and summary["passes"] <= 4
    assert sum(summary["pass_tiles"]) == summary["n_tiles"] == len(tiles)
    assert all(summary["pass_tiles"][p] > 0 for p in range(summary["passes"]))
    assert all(summary["pass_tiles"][p] == 0 for p in range(summary["passes"], 4))
    tree = [None] * summary["tree_rows"]
    read_pass0 = bytearray(len(rows))
    for p in range(summary["passes"]):
        pad = _pad(height + 9 * p)
        src = rows if p == 0 else tree
        written = []  # a launch's own stores become visible to the next launch only

        def store(row0, level):
            assert 0 <= row0 and row0 + len(level) <= len(tree), "a store reaches past the tree"
            written.extend((row0 + k, r) for k, r in enumerate(level))

        for tp, src_row, dst_row, level_rows, tile in tiles:
            if tp != p:
                continue
            pos = 512 * tile
            assert level_rows >= 1 and pos < level_rows
            n = min(512, level_rows - pos)
            levels = 9 if level_rows > 512 else (level_rows - 1).bit_length()
            assert p == 0 or src_row == dst_row, "a later pass reads the tree where the pass before wrote it"
            assert src_row + pos + n <= len(src), "a row index reaches past the input"
            level = src[src_row + pos:src_row + pos + n]
            assert None not in level, "a tree row is read before the launch that writes it"
            if p == 0:
                assert not any(read_pass0[src_row + pos:src_row + pos + n]), "an input row belongs to two tiles"
                read_pass0[src_row + pos:src_row + pos + n] = b"\x01" * n
                store(dst_row + pos, level)
            level = level + [pad] * (512 - n)
            base, width = dst_row, level_rows
            for j in range(1, levels + 1):
                level = [_sha(level[k], level[k + 1]) for k in range(0, (1 << levels) >> (j - 1), 2)]
                base += width
                width = (width + 1) >> 1
                pos >>= 1
                store(base + pos, level[:(n + (1 << j) - 1) >> j])
        for row, value in written:
            assert tree[row] is None, "a tree row is written twice"
            tree[row] = value
    assert all(read_pass0), "an input row belongs to no tile"
    assert None not in tree, "a tree row is never written"
    return tree


def _check_against_build_tree(counts, rows, height):
    from vortex_amd import merkle

    summary, tiles, off = _plan(counts)
    assert off[0] == 0 and off[-1] == summary["tree_rows"] == sum(merkle.tree_rows(c) for c in counts)
    tree = replay(summary, tiles, rows, height)
    at = 0
    for f, c in enumerate(counts):
        assert off[f + 1] - off[f] == merkle.tree_rows(c)
        want = merkle.build_tree(rows[at:at + c], height)
        assert b"".join(tree[off[f]:off[f + 1]]) == want, f"layer {f} of {c} rows"
        assert tree[off[f + 1] - 1] == merkle.layer_root(rows[at:at + c], height)  # the last row is the root
        at += c
    return summary


@pytest.mark.parametrize("height", [0, 4])
def test_planner_replay_matches_build_tree(built, layer_rows, height):
    summary = _check_against_build_tree(COUNTS, layer_rows, height)
    assert summary["passes"] == 3 and summary["rows"] == sum(COUNTS)


@pytest.mark.parametrize("height", [0, 4])
@pytest.mark.parametrize("count", COUNTS)
def test_planner_replay_of_each_count_alone(built, layer_rows, count, height):
    _check_against_build_tree([count], layer_rows[:count], height)


def test_build_tree_is_the_tree_model():
    """merkle.build_tree: node (k, j) of merkle._Tree is row j of level k, pad
    hashes are not stored, tree_rows counts the rows, and a wrong pad height
    shows."""
    from vortex_amd import merkle

    rng = random.Random(3)
    assert [merkle.tree_rows(m) for m in (0, 1, 2, 3, 5, 512, 513)] == [0, 1, 3, 6, 11, 1023, 1034]
    for m in (1, 2, 3, 5, 8, 9, 33):
        rows = [rng.randbytes(32) for _ in range(m)]
        for height in (0, 3):
            tree = merkle.build_tree(rows, height)
            assert len(tree) == 32 * merkle.tree_rows(m) <= 32 * (2 * m + (m - 1).bit_length())
            model = merkle._Tree(rows, height)
            at = 0
            for k in range((m - 1).bit_length() + 1):
                n_k = (m + (1 << k) - 1) >> k
                for j in range(n_k):
                    assert tree[at:at + 32] == model.node(k, j), (m, k, j)
                    at += 32
            assert at == len(tree) and tree[-32:] == merkle.layer_root(rows, height)
        if m & (m - 1):  # a level of odd length takes a pad hash: its height matters
            assert merkle.build_tree(rows, 0)[-32:] != merkle.build_tree(rows, 1)[-32:]
    with pytest.raises(ValueError):
        merkle.build_tree(b"", 0)


# ---- the planner as a stand-alone program under ASan+UBSan ----------------------

@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("mtp") / "merkle_tree_plan_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "merkle_tree_plan_dump.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, mode, counts):
    out = subprocess.run([str(exe), mode], input="\n".join(map(str, counts)) + "\n", capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.rstrip("\n").split("\n")


@pytest.mark.parametrize("counts", [COUNTS] + [[c] for c in COUNTS], ids=lambda c: "all" if len(c) > 1 else str(c[0]))
def test_planner_standalone_under_sanitizers(built, plan_exe, counts):
    lines = _run(plan_exe, "dump", counts)
    summary = json.loads(lines[-1])
    tiles = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("T ")]
    off = [int(ln.split()[1]) for ln in lines if ln.startswith("O ")]
    assert len(tiles) + len(off) + 1 == len(lines)
    assert (summary, tiles, off) == _plan(counts)  # the library's planner is this header


def test_standalone_refusals(plan_exe):
    """The planner, the layout and the proof lookup: what they refuse, that a
    refused call writes nothing, and that no accepted one reads or writes past
    buffers of exactly the documented size."""
    assert _run(plan_exe, "errors", COUNTS) == ["ok"]


# ---- proofs out of a tree ---------------------------------------------------------

def walk(rows, span, uncles, pos):
    """A receiver's check of one `hashes` message: ten lines of hashlib."""
    level = [rows[32 * k:32 * k + 32] for k in range(span)]
    while len(level) > 1:
        level = [_sha(level[k], level[k + 1]) for k in range(0, len(level), 2)]
    cur = level[0]
    for k in range(uncles):
        u = rows[32 * (span + k):32 * (span + k) + 32]
        cur = _sha(u, cur) if (pos >> k) & 1 else _sha(cur, u)
    return cur


@pytest.mark.parametrize("m", [1, 3, 512, 513, 1025])
def test_tree_proof_equals_make_proof(built, m):
    """Every (level, span, pos, uncles) with span in {1, 2, 512} and uncles from
    0 to two past the root, through the library: equal to merkle.make_proof over
    that level's rows, and reducing to the layer's root under a plain walk."""
    from vortex_amd import _lib, merkle

    L = _lib.lib()
    rng = random.Random(m)
    height = 2
    rows = [rng.randbytes(32) for _ in range(m)]
    tree = merkle.build_tree(rows, height)
    root = merkle.layer_root(rows, height)
    K = (m - 1).bit_length()
    out = ctypes.create_string_buffer(32 * (512 + 64))
    at = 0
    checked = 0
    for level in range(K + 1):
        n_level = (m + (1 << level) - 1) >> level
        level_rows = tree[32 * at:32 * (at + n_level)]
        at += n_level
        for span in (1, 2, 512):
            log_span = span.bit_length() - 1
            to_root = max(K - level - log_span, 0)
            for pos in range(-(-n_level // span)):
                # (make_proof builds its tree anew on every call: once per position, at the longest walk;
                # a shorter proof is its prefix, which test_merkle_layers_cpu checks of make_proof itself)
                want = merkle.make_proof(level_rows, height + level, pos, span, to_root + 2)
                for uncles in range(to_root + 3):
                    assert L.vx_merkle_tree_proof(tree, m, height, level, pos, span, uncles, out) == 0
                    got = out.raw[:32 * (span + uncles)]
                    assert got == want[:32 * (span + uncles)], (level, span, pos, uncles)
                    checked += 1
                assert merkle.proof_from_tree(tree, m, height, level, pos, span, to_root) == want[:32 * (span + to_root)]
                if level + log_span <= K:
                    assert walk(want, span, to_root, pos) == root, (level, span, pos)
                else:  # a span wider than the layer: its root is the layer's root under pad hashes
                    top = root
                    for k in range(K, level + log_span):
                        top = _sha(top, _pad(height + k))
                    assert walk(want, span, 0, pos) == top
    assert checked >= 3 * (K + 1)


def test_tree_proof_refusals(built):
    from vortex_amd import _lib, merkle

    L = _lib.lib()
    rows = [bytes([k]) * 32 for k in range(5)]
    tree = merkle.build_tree(rows, 0)
    out = ctypes.create_string_buffer(32 * 600)

    def proof(tree=tree, m=5, height=0, level=0, pos=0, span=1, uncles=0, out=out):
        return L.vx_merkle_tree_proof(tree, m, height, level, pos, span, uncles, out)

    assert proof() == 0 and out.raw[:32] == rows[0]
    for span in (0, 3, 6, 513, 1024):
        assert proof(span=span) == _lib.VX_EINVAL and b"span" in L.vx_last_error()
    assert proof(uncles=65) == _lib.VX_EINVAL and proof(uncles=64) == 0
    assert proof(level=4) == _lib.VX_EINVAL and proof(level=3) == 0 and out.raw[:32] == tree[-32:]
    assert proof(pos=5) == _lib.VX_EINVAL and proof(pos=4) == 0
    assert proof(span=4, pos=2) == _lib.VX_EINVAL and proof(span=4, pos=1) == 0
    assert out.raw[:128] == rows[4] + bytes(96)  # rows past the layer: pad(0)
    assert proof(m=0) == _lib.VX_EINVAL and proof(height=65) == _lib.VX_EINVAL
    assert proof(tree=None) == _lib.VX_EINVAL and proof(out=None) == _lib.VX_EINVAL
    with pytest.raises(ValueError):
        merkle.proof_from_tree(tree[:-32], 5, 0, 0, 0, 1, 0)


# ---- the layout of a torrent's trees ----------------------------------------------

@pytest.mark.parametrize("pl", [16384, 65536])
def test_tree_layout_matches_the_model(built, pl):
    from vortex_amd import _lib, merkle

    L = _lib.lib()
    layouts = [[], [0], [0, 0], [1], [pl], [pl - 1], [pl + 1], [0, pl, 0, pl + 1, pl - 1, 1, 0],
               [5 * pl, 0, 513 * pl - 5, 2 * pl, 2 * pl + 1, 3], [200000, 1, 65537, 100000, 0, 49152]]
    for flens in layouts:
        n = len(flens)
        arr = (ctypes.c_uint64 * max(n, 1))(*flens)
        counts = (ctypes.c_uint32 * max(n, 1))()
        off = (ctypes.c_uint64 * (n + 1))()
        total = L.vx_merkle_tree_layout(arr, n, pl, counts, off)
        want_counts, want_off = merkle.tree_layout(flens, pl)
        assert (list(counts)[:n], list(off), total) == (want_counts, want_off, want_off[-1]), flens
        assert L.vx_merkle_tree_layout(arr, n, pl, None, None) == total
        # a file's rows are its pieces: 0 for an empty file, 1 up to piece_length, one per piece above
        assert want_counts == [len(merkle.file_pieces(x, pl)[0]) for x in flens]
        assert all(L.vx_merkle_tree_rows(c) == merkle.tree_rows(c) == b - a
                   for c, a, b in zip(want_counts, want_off, want_off[1:]))
    one = (ctypes.c_uint64 * 1)(5)
    for bad in (0, 16383, 16385, 3 * 16384):
        assert L.vx_merkle_tree_layout(one, 1, bad, None, None) == _lib.VX_EINVAL
        assert b"piece_length" in L.vx_last_error()
    assert L.vx_merkle_tree_layout(None, 1, 16384, None, None) == _lib.VX_EINVAL
    with pytest.raises(ValueError):
        merkle.tree_layout([5], 16385)


# ---- what the entries refuse before they touch a device ---------------------------

def test_validation_without_gpu(built):
    from vortex_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p

    def einval(rc, word):
        assert rc == _lib.VX_EINVAL, rc
        assert word in L.vx_last_error(), L.vx_last_error()

    # the planner
    counts = (ctypes.c_uint32 * 3)(5, 600, 1)
    plan = _lib.vx_merkle_tree_plan()
    einval(L.vx_merkle_tree_plan(counts, 3, None, None, 0, None), b"NULL")
    einval(L.vx_merkle_tree_plan(None, 3, ctypes.byref(plan), None, 0, None), b"NULL")
    assert L.vx_merkle_tree_plan(None, 0, ctypes.byref(plan), None, 0, None) == 0
    assert (plan.n_layers, plan.passes, plan.rows, plan.tree_rows, plan.n_tiles) == (0, 0, 0, 0, 0)
    einval(L.vx_merkle_tree_plan((ctypes.c_uint32 * 3)(5, 0, 1), 3, ctypes.byref(plan), None, 0, None), b"count is 0")
    einval(L.vx_merkle_tree_plan((ctypes.c_uint32 * 2)(1 << 31, 1 << 31), 2, ctypes.byref(plan), None, 0, None), b"2^32")
    einval(L.vx_merkle_tree_plan((ctypes.c_uint32 * 1)((1 << 31) + 1), 1, ctypes.byref(plan), None, 0, None), b"2^32")
    assert L.vx_merkle_tree_plan(counts, 3, ctypes.byref(plan), None, 0, None) == 0
    # 5 rows: 5+3+2+1; 600 rows: 600+300+150+75+38+19+10+5+3+2+1; 1 row
    assert (plan.n_layers, plan.passes, plan.rows, plan.tree_rows, plan.n_tiles, list(plan.pass_tiles)) == \
        (3, 2, 606, 11 + 1203 + 1, 5, [4, 1, 0, 0])
    tiles = (_lib.vx_merkle_tree_tile * 6)()
    ctypes.memset(tiles, 0xA5, ctypes.sizeof(tiles))
    einval(L.vx_merkle_tree_plan(counts, 3, ctypes.byref(plan), tiles, 4, None), b"tiles_cap")
    assert bytes(tiles) == b"\xA5" * ctypes.sizeof(tiles)  # nothing written
    assert L.vx_merkle_tree_plan(counts, 3, ctypes.byref(plan), tiles, 5, None) == 0
    assert bytes(tiles)[5 * 16:] == b"\xA5" * 16
    got = [(t.src_row, t.dst_row, t.level_rows, t.tile) for t in tiles[:5]]
    # layer 1's level 9 starts 600+300+...+3 = 1200 rows into its tree, which starts at row 11
    assert got == [(0, 0, 5, 0), (5, 11, 600, 0), (5, 11, 600, 1), (605, 1214, 1, 0), (1211, 1211, 2, 0)]

    # the device entry: checked on the host, no device touched
    hashes, d_tiles, tree = p(0x10000), p(0x20000), p(0x100000)
    pl = ctypes.byref(plan)

    def trees(hashes=hashes, pl=pl, d_tiles=d_tiles, height=4, tree=tree):
        return L.vx_merkle_device_trees(hashes, pl, d_tiles, height, tree, None)

    einval(trees(pl=None), b"NULL plan")
    einval(trees(hashes=None), b"NULL")
    einval(trees(d_tiles=None), b"NULL")
    einval(trees(tree=None), b"NULL")
    einval(trees(height=65), b"height > 64")
    einval(trees(hashes=p(0x10008)), b"aligned")
    einval(trees(tree=p(0x100008)), b"aligned")
    einval(trees(d_tiles=p(0x20002)), b"aligned")
    einval(trees(tree=p(0x10000 + 32 * 605)), b"overlaps")  # the tree's first row is the layers' last
    einval(trees(tree=p(0x10000 - 32 * 1214)), b"overlaps")  # the tree's last row is the layers' first
    bad = _lib.vx_merkle_tree_plan.from_buffer_copy(plan)
    bad.passes = 5
    einval(trees(pl=ctypes.byref(bad)), b"not a plan")
    bad.passes, bad.n_tiles = 2, 6
    einval(trees(pl=ctypes.byref(bad)), b"not a plan")
    bad.n_tiles, bad.tree_rows = 5, 605
    einval(trees(pl=ctypes.byref(bad)), b"not a plan")
    empty = _lib.vx_merkle_tree_plan()
    assert L.vx_merkle_device_trees(None, ctypes.byref(empty), None, 0, None, None) == 0

    # the host entries: a NULL context first; the rest with a context pointer
    # the entry must not reach, since every case fails on its arguments alone
    hbuf = ctypes.create_string_buffer(32 * 606)
    tbuf = ctypes.create_string_buffer(32 * 1215)
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, p)

    def build(ctx=ctx, hashes=hbuf, counts=counts, n=3, height=4, tree=tbuf):
        return L.vx_merkle_build_trees(ctx, hashes, counts, n, height, tree, None)

    einval(build(ctx=None), b"NULL context")
    for k in ("hashes", "counts", "tree"):
        einval(build(**{k: None}), b"NULL")
    einval(build(height=65), b"height > 64")
    einval(build(counts=(ctypes.c_uint32 * 3)(5, 0, 1)), b"count is 0")
    einval(build(counts=(ctypes.c_uint32 * 3)(1 << 31, 1 << 31, 1)), b"2^32")
    assert build(n=0) == 0 and build(n=0, hashes=None, counts=None, tree=None) == 0

    # the three hash calls: a bad n_pieces, a wrong tree_rows, a bad range, NULL outputs
    pl_bytes = 65536
    flens = (ctypes.c_uint64 * 3)(3 * pl_bytes + 1, 0, 5)  # v1: 4 pieces; v2 and hybrid: 4 + 0 + 1
    paths = (ctypes.c_char_p * 3)(b"a", b"b", b"c")
    dig, rows, ok = ctypes.create_string_buffer(20 * 5), ctypes.create_string_buffer(32 * 5), ctypes.create_string_buffer(5)
    rows_of_trees = L.vx_merkle_tree_layout(flens, 3, pl_bytes, None, None)
    assert rows_of_trees == (4 + 2 + 1) + 0 + 1
    big = ctypes.create_string_buffer(32 * 8)
    einval(L.vx_hash_files(None, paths, flens, 3, pl_bytes, 4, dig, ok, 0), b"NULL context")
    einval(L.vx_hash_files(ctx, paths, flens, 3, pl_bytes, 5, dig, ok, 0), b"n_pieces")
    einval(L.vx_hash_files(ctx, paths, flens, 3, pl_bytes, 4, None, ok, 0), b"NULL")
    einval(L.vx_hash_files(ctx, paths, flens, 3, 0, 4, dig, ok, 0), b"piece_length")
    einval(L.vx_hash_files_range(ctx, paths, flens, 3, pl_bytes, 4, 3, 2, dig, ok, 0), b"range")
    einval(L.vx_merkle_hash_files(None, paths, flens, 3, pl_bytes, 5, rows, ok, big, 8, 0), b"NULL context")
    einval(L.vx_merkle_hash_files(ctx, paths, flens, 3, pl_bytes, 4, rows, ok, big, 8, 0), b"n_pieces")
    einval(L.vx_merkle_hash_files(ctx, paths, flens, 3, pl_bytes, 5, rows, ok, big, 7, 0), b"tree_rows")
    einval(L.vx_merkle_hash_files(ctx, paths, flens, 3, pl_bytes, 5, rows, ok, big, 9, 0), b"tree_rows")
    einval(L.vx_merkle_hash_files(ctx, paths, flens, 3, pl_bytes, 5, None, ok, big, 8, 0), b"NULL")
    einval(L.vx_merkle_hash_files(ctx, paths, flens, 3, 3 * 16384, 5, rows, ok, big, 8, 0), b"piece_length")
    einval(L.vx_merkle_hash_files_range(ctx, paths, flens, 3, pl_bytes, 5, 4, 2, rows, ok, 0), b"range")
    einval(L.vx_merkle_hash_files_range(ctx, paths, flens, 3, pl_bytes, 6, 0, 1, rows, ok, 0), b"n_pieces")
    einval(L.vx_hybrid_hash_files(None, paths, flens, 3, pl_bytes, 5, dig, rows, ok, big, 8, 0), b"NULL context")
    einval(L.vx_hybrid_hash_files(ctx, paths, flens, 3, pl_bytes, 4, dig, rows, ok, big, 8, 0), b"n_pieces")
    einval(L.vx_hybrid_hash_files(ctx, paths, flens, 3, pl_bytes, 5, dig, rows, ok, big, 7, 0), b"tree_rows")
    einval(L.vx_hybrid_hash_files(ctx, paths, flens, 3, pl_bytes, 5, None, rows, ok, big, 8, 0), b"NULL")
    einval(L.vx_hybrid_hash_files(ctx, paths, flens, 3, pl_bytes, 5, dig, None, ok, big, 8, 0), b"NULL")
    einval(L.vx_hybrid_hash_files_range(ctx, paths, flens, 3, pl_bytes, 5, 5, 1, dig, rows, ok, 0), b"range")
    einval(L.vx_hybrid_hash_files_range(ctx, paths, flens, 3, pl_bytes, 4, 0, 1, dig, rows, ok, 0), b"n_pieces")


# ---- INTEGRATION.md -----------------------------------------------------------------

def test_rust_binding_of_the_new_entries_matches_the_header(monkeypatch):
    """The `extern "C"` lines and `#[repr(C)]` structs INTEGRATION.md gives for
    the new entries, against include/vx_hash.h, with test_integration_doc's
    parsers (that test reads the document's first Rust block only)."""
    import re

    import test_integration_doc as doc

    names = {"VxMerkleTreeTile": "vx_merkle_tree_tile", "VxMerkleTreePlan": "vx_merkle_tree_plan"}
    for k, v in names.items():
        monkeypatch.setitem(doc.RUST_TO_C, k, v)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = next(b for b in re.findall(r"```rust\n(.*?)```", text, flags=re.S) if "vx_merkle_tree_plan" in b)
    monkeypatch.setattr(doc, "rust_block", lambda: block)
    rust, c = doc.rust_externs(), doc.c_prototypes()
    assert set(rust) == NEW

    def untagged(t):  # C names the plan by its tag: `struct vx_merkle_tree_plan`, const or not
        return t.replace("structc vx_merkle_tree_plan", "vx_merkle_tree_planc").replace("struct ", "")

    for name, (ret, args) in rust.items():
        cret, cargs = c[name]
        assert ret == cret and args == [untagged(a) for a in cargs], (name, args, cargs)
    structs, cstructs = doc.rust_structs(), doc.c_structs()
    assert structs["VxMerkleTreeTile"] == cstructs["vx_merkle_tree_tile"]
    from vortex_amd import _lib

    ctype_names = {ctypes.c_uint32: "uint32_t", ctypes.c_uint64: "uint64_t", ctypes.c_uint32 * 4: "uint32_t[4]"}
    assert structs["VxMerkleTreePlan"] == [(n, ctype_names[t]) for n, t in _lib.vx_merkle_tree_plan._fields_]
