"""CPU: v2 `piece layers` and hash proofs in batches — the five new C ABI
entries (header, struct layouts, exports, argument validation), the planner
of vx_merkle_device_layers replayed in Python with hashlib against the direct
BEP 52 model and run as a stand-alone program under ASan+UBSan
(vortex_amd/csrc/vx_merkle_layers.hpp), and merkle.layer_counts / layer_root /
make_proof against a pure-Python tree.  No GPU, no compute calls."""
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

NEW = {"vx_merkle_layers_plan", "vx_merkle_device_layers", "vx_merkle_device_proofs", "vx_merkle_verify_layers",
       "vx_merkle_verify_proofs"}
# one, two and three passes, and every edge of a tile
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 262144, 262145]


def _sha(a, b):
    return hashlib.sha256(a + b).digest()


def _pad(height):
    h = bytes(32)
    for _ in range(height):
        h = _sha(h, h)
    return h


def model_root(rows, height):
    """BEP 52: pad the layer to a power of two with pad(height), reduce
    pairwise.  (A subtree of padding alone is the pad hash one level up, so a
    level of odd length gets one pad hash of its own height instead of the
    padding being hashed out row by row.)"""
    level = list(rows)
    for k in range((len(rows) - 1).bit_length()):
        if len(level) & 1:
            level.append(_pad(height + k))
        level = [_sha(level[j], level[j + 1]) for j in range(0, len(level), 2)]
    assert len(level) == 1
    return level[0]


# ---- header, layouts, exports, validation ------------------------------------

def test_header_declares_the_new_entries_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "int main(void){\n"
                 "  int (*a)(const uint32_t*, uint32_t, struct vx_merkle_layers_plan*, vx_merkle_tile*, size_t)"
                 " = vx_merkle_layers_plan;\n"
                 "  int (*b)(const void*, const struct vx_merkle_layers_plan*, const vx_merkle_tile*, uint32_t, void*,"
                 " void*, const void*, void*, void*) = vx_merkle_device_layers;\n"
                 "  int (*c)(const void*, const vx_merkle_proof*, uint32_t, void*, const void*, void*, void*)"
                 " = vx_merkle_device_proofs;\n"
                 "  int (*d)(vx_ctx*, const uint8_t*, const uint32_t*, uint32_t, uint32_t, const uint8_t*, uint8_t*,"
                 " uint8_t*) = vx_merkle_verify_layers;\n"
                 "  int (*e)(vx_ctx*, const uint8_t*, uint64_t, const vx_merkle_proof*, uint32_t, const uint8_t*,"
                 " uint32_t, uint8_t*, uint8_t*) = vx_merkle_verify_proofs;\n"
                 "  (void)a; (void)b; (void)c; (void)d; (void)e;\n"
                 "  return VX_ABI_VERSION != 3 || VX_MERKLE_TILE_ROWS != 512; }\n")
    for compiler, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        if shutil.which(compiler) is None:
            continue
        src = c if compiler == "gcc" else tmp_path / "t.cpp"
        if src != c:
            src.write_text(c.read_text())
        subprocess.run([compiler, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], check=True)


@pytest.mark.parametrize("struct,ctype,size", [
    ("vx_merkle_tile", "vx_merkle_tile", 16),
    ("vx_merkle_layers_plan", "struct vx_merkle_layers_plan", 48),
    ("vx_merkle_proof", "vx_merkle_proof", 24)])
def test_struct_layouts(tmp_path, struct, ctype, size):
    """The three structs as ctypes have the C layout: size and every field's
    offset; C says so, compiled here."""
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
    assert got[0] == size


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


def test_validation_without_gpu(built):
    """Everything the five entries refuse before they touch a device."""
    from vortex_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p

    def einval(rc, word):
        assert rc == _lib.VX_EINVAL, rc
        assert word in L.vx_last_error(), L.vx_last_error()

    # the planner
    counts = (ctypes.c_uint32 * 3)(5, 600, 1)
    plan = _lib.vx_merkle_layers_plan()
    einval(L.vx_merkle_layers_plan(counts, 3, None, None, 0), b"NULL")
    einval(L.vx_merkle_layers_plan(None, 3, ctypes.byref(plan), None, 0), b"NULL")
    assert L.vx_merkle_layers_plan(None, 0, ctypes.byref(plan), None, 0) == 0
    assert (plan.n_layers, plan.passes, plan.rows, plan.work_rows, plan.n_tiles) == (0, 0, 0, 0, 0)
    einval(L.vx_merkle_layers_plan((ctypes.c_uint32 * 3)(5, 0, 1), 3, ctypes.byref(plan), None, 0), b"count is 0")
    einval(L.vx_merkle_layers_plan((ctypes.c_uint32 * 2)(1 << 31, 1 << 31), 2, ctypes.byref(plan), None, 0), b"2^32")
    assert L.vx_merkle_layers_plan(counts, 3, ctypes.byref(plan), None, 0) == 0
    assert (plan.n_layers, plan.passes, plan.rows, plan.work_rows, plan.n_tiles, list(plan.pass_tiles)) == \
        (3, 2, 606, 2, 5, [4, 1, 0, 0])
    tiles = (_lib.vx_merkle_tile * 6)()
    ctypes.memset(tiles, 0xA5, ctypes.sizeof(tiles))
    einval(L.vx_merkle_layers_plan(counts, 3, ctypes.byref(plan), tiles, 4), b"tiles_cap")
    assert bytes(tiles) == b"\xA5" * ctypes.sizeof(tiles)  # nothing written
    assert L.vx_merkle_layers_plan(counts, 3, ctypes.byref(plan), tiles, 5) == 0
    assert bytes(tiles)[5 * 16:] == b"\xA5" * 16
    got = [(t.in_row, t.out, t.rows, t.levels, t.last) for t in tiles[:5]]
    assert got == [(0, 0, 5, 3, 1), (5, 0, 512, 9, 0), (517, 1, 88, 9, 0), (605, 2, 1, 0, 1), (0, 1, 2, 1, 1)]

    # the device entries: checked on the host, no device touched
    hashes, d_tiles, work, roots, exp, match = p(0x10000), p(0x20000), p(0x30000), p(0x40000), p(0x50000), p(0x60000)
    pl = ctypes.byref(plan)

    def layers(hashes=hashes, pl=pl, d_tiles=d_tiles, height=4, work=work, roots=roots, exp=exp, match=match):
        return L.vx_merkle_device_layers(hashes, pl, d_tiles, height, work, roots, exp, match, None)

    einval(layers(pl=None), b"NULL plan")
    einval(layers(hashes=None), b"NULL")
    einval(layers(d_tiles=None), b"NULL")
    einval(layers(work=None), b"NULL")  # this plan has work rows
    einval(layers(height=65), b"height > 64")
    einval(layers(hashes=p(0x10008)), b"aligned")
    einval(layers(work=p(0x30008)), b"aligned")
    einval(layers(roots=p(0x40004)), b"aligned")
    einval(layers(d_tiles=p(0x20002)), b"aligned")
    einval(layers(exp=p(0x50001)), b"aligned")
    bad = _lib.vx_merkle_layers_plan.from_buffer_copy(plan)
    bad.passes = 5
    einval(layers(pl=ctypes.byref(bad)), b"not a plan")
    bad.passes, bad.n_tiles = 2, 6
    einval(layers(pl=ctypes.byref(bad)), b"not a plan")
    empty = _lib.vx_merkle_layers_plan()
    assert L.vx_merkle_device_layers(None, ctypes.byref(empty), None, 0, None, None, None, None, None) == 0

    proofs, tops = p(0x20000), p(0x30000)

    def dproofs(hashes=hashes, proofs=proofs, n=4, tops=tops, exp=exp, match=match):
        return L.vx_merkle_device_proofs(hashes, proofs, n, tops, exp, match, None)

    for k in ("hashes", "proofs", "tops", "exp", "match"):
        einval(dproofs(**{k: None}), b"NULL")
    einval(dproofs(hashes=p(0x10008)), b"aligned")
    einval(dproofs(tops=p(0x30008)), b"aligned")
    einval(dproofs(proofs=p(0x20004)), b"aligned")
    einval(dproofs(exp=p(0x50002)), b"aligned")
    assert L.vx_merkle_device_proofs(None, None, 0, None, None, None, None) == 0  # n == 0 launches nothing

    # the host entries: a NULL context first; the rest with a context pointer
    # the entry must not reach, since every case fails on its arguments alone
    hbuf = ctypes.create_string_buffer(32 * 606)
    ebuf = ctypes.create_string_buffer(32 * 3)
    out = ctypes.create_string_buffer(8)
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, p)

    def vlayers(ctx=ctx, hashes=hbuf, counts=counts, n=3, height=4, exp=ebuf, out=out):
        return L.vx_merkle_verify_layers(ctx, hashes, counts, n, height, exp, out, None)

    einval(vlayers(ctx=None), b"NULL context")
    for k in ("hashes", "counts", "exp", "out"):
        einval(vlayers(**{k: None}), b"NULL")
    einval(vlayers(height=65), b"height > 64")
    einval(vlayers(counts=(ctypes.c_uint32 * 3)(5, 0, 1)), b"count is 0")
    einval(vlayers(counts=(ctypes.c_uint32 * 3)(1 << 31, 1 << 31, 1)), b"2^32")
    assert vlayers(n=0) == 0 and vlayers(n=0, hashes=None, counts=None, exp=None, out=None) == 0

    def vproofs(plist, ctx=ctx, hashes=hbuf, n_rows=606, exp=ebuf, n_exp=3, out=out, n=None):
        arr = _lib.proof_array(plist)
        return L.vx_merkle_verify_proofs(ctx, hashes, n_rows, arr, len(plist) if n is None else n, exp, n_exp, out,
                                         None)

    good = (0, 0, 0, 4, 3)  # (pos, row, expected, span, uncles)
    einval(vproofs([good], ctx=None), b"NULL context")
    for k in ("hashes", "exp", "out"):
        einval(vproofs([good], **{k: None}), b"NULL")
    einval(L.vx_merkle_verify_proofs(ctx, hbuf, 606, None, 1, ebuf, 3, out, None), b"NULL")
    assert vproofs([], n=0) == 0
    for span in (0, 3, 6, 1024, 513):
        einval(vproofs([good, good, (0, 0, 0, span, 3)]), b"proof 2: span")
    assert b"proof 2" in L.vx_last_error()
    einval(vproofs([good, (0, 0, 0, 4, 65), (0, 0, 0, 3, 3)]), b"proof 1: uncles")  # the first bad index
    einval(vproofs([(0, 600, 0, 4, 3)]), b"proof 0: row + span + uncles")
    einval(vproofs([(0, 0xFFFFFFFF, 0, 512, 64)]), b"proof 0: row + span + uncles")  # no 32-bit wrap
    einval(vproofs([good, (0, 599, 0, 4, 3), (0, 0, 3, 4, 3)]), b"proof 2: expected")
    einval(vproofs([(0, 0, 0, 1, 0)], n_exp=0), b"proof 0: expected")


# ---- the planner, replayed -----------------------------------------------------

def _plan(counts):
    from vortex_amd import _lib

    L = _lib.lib()
    carr = (ctypes.c_uint32 * len(counts))(*counts)
    plan = _lib.vx_merkle_layers_plan()
    assert L.vx_merkle_layers_plan(carr, len(counts), ctypes.byref(plan), None, 0) == 0
    tiles = (_lib.vx_merkle_tile * plan.n_tiles)()
    assert L.vx_merkle_layers_plan(carr, len(counts), ctypes.byref(plan), tiles, plan.n_tiles) == 0
    summary = {"n_layers": plan.n_layers, "passes": plan.passes, "rows": plan.rows, "work_rows": plan.work_rows,
               "n_tiles": plan.n_tiles, "pass_tiles": list(plan.pass_tiles)}
    at, out = 0, []
    for p in range(plan.passes):
        for _ in range(plan.pass_tiles[p]):
            t = tiles[at]
            assert t._pad == 0
            out.append((p, t.in_row, t.out, t.rows, t.levels, t.last))
            at += 1
    return summary, out


@pytest.fixture(scope="module")
def layer_rows():
    """The input of every replay: random rows, as many as the counts need (built once)."""
    rng = random.Random(0x1A7E25)
    blob = rng.randbytes(32 * sum(COUNTS))
    return [blob[k:k + 32] for k in range(0, len(blob), 32)]


def replay(summary, tiles, counts, rows, height):
    """Execute the tiles pass by pass with hashlib, as merkle_layers_kernel
    does, and check what the plan promises about its rows on the way."""
    assert summary["n_layers"] == len(counts) and summary["rows"] == sum(counts) == len(rows)
    assert sum(summary["pass_tiles"]) == summary["n_tiles"] == len(tiles) and summary["passes"] <= 4
    assert all(summary["pass_tiles"][p] > 0 for p in range(summary["passes"]))
    assert all(summary["pass_tiles"][p] == 0 for p in range(summary["passes"], 4))
    work = [None] * summary["work_rows"]
    roots = [None] * len(counts)
    read_pass0 = bytearray(len(rows))
    for p in range(summary["passes"]):
        pad = _pad(height + 9 * p)
        src = rows if p == 0 else work
        limit = summary["rows"] if p == 0 else summary["work_rows"]
        written = []
        for tp, in_row, out, n, levels, last in tiles:
            if tp != p:
                continue
            assert 1 <= n <= 512 and 0 <= levels <= 9 and n <= 1 << levels and last in (0, 1)
            assert in_row + n <= limit, "a row index reaches past the input"
            level = src[in_row:in_row + n]
            assert None not in level, "a work row is read before it is written"
            if p == 0:
                assert not any(read_pass0[in_row:in_row + n]), "an input row belongs to two tiles"
                read_pass0[in_row:in_row + n] = b"\x01" * n
            level = level + [pad] * ((1 << levels) - n)
            while len(level) > 1:
                level = [_sha(level[k], level[k + 1]) for k in range(0, len(level), 2)]
            if last:
                assert 0 <= out < len(counts) and roots[out] is None, "a layer has two roots"
                roots[out] = level[0]
            else:
                assert levels == 9 and 0 <= out < summary["work_rows"]
                written.append((out, level[0]))
        # a launch's own outputs become visible to the next launch only
        for out, row in written:
            assert work[out] is None, "a work row is written twice"
            work[out] = row
    assert all(read_pass0), "an input row belongs to no tile"
    assert None not in work and None not in roots
    return roots


@pytest.mark.parametrize("height", [0, 4])
def test_planner_replay_matches_bep52(built, layer_rows, height):
    summary, tiles = _plan(COUNTS)
    assert summary["passes"] == 3
    roots = replay(summary, tiles, COUNTS, layer_rows, height)
    at = 0
    for f, c in enumerate(COUNTS):
        assert roots[f] == model_root(layer_rows[at:at + c], height), f"layer {f} of {c} rows"
        at += c


def test_planner_pass_rule(built):
    """launch_merkle_root's rule per layer: m <= 512 is one last tile of
    ceil(log2 m) levels, otherwise ceil(m / 512) tiles of 9 levels."""
    summary, tiles = _plan(COUNTS)
    alive = list(COUNTS)
    for p in range(summary["passes"]):
        mine = [t for t in tiles if t[0] == p]
        want = []
        for f, m in enumerate(alive):
            if m is None:
                continue
            if m <= 512:
                want.append((m, (m - 1).bit_length(), 1, f))
                alive[f] = None
            else:
                k = -(-m // 512)
                want += [(min(512, m - 512 * j), 9, 0, None) for j in range(k)]
                alive[f] = k
        assert [(t[3], t[4], t[5]) for t in mine] == [w[:3] for w in want]
        assert [t[2] for t in mine if t[5]] == [w[3] for w in want if w[2]]
    assert all(m is None for m in alive)


# ---- the planner as a stand-alone program under ASan+UBSan --------------------

@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("mlp") / "merkle_layers_plan_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "merkle_layers_plan_dump.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, mode, counts):
    out = subprocess.run([str(exe), mode], input="\n".join(map(str, counts)) + "\n", capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.rstrip("\n").split("\n")


def test_planner_standalone_under_sanitizers(built, plan_exe):
    lines = _run(plan_exe, "dump", COUNTS)
    summary = json.loads(lines[-1])
    tiles = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[:-1]]
    assert all(ln.startswith("T ") for ln in lines[:-1])
    assert (summary, tiles) == _plan(COUNTS)  # the library's planner is this header


def test_planner_standalone_refusals(plan_exe):
    """A zero count, a sum of 2^32, tiles_cap = n_tiles - 1 with a guard region
    behind the array: refused, nothing written."""
    assert _run(plan_exe, "errors", COUNTS) == ["ok"]


# ---- merkle.py ----------------------------------------------------------------

def test_layer_counts():
    from vortex_amd import merkle

    pl = 65536
    flens = [0, 1, pl, pl + 1, 2 * pl, 2 * pl + 1, 5, 100 * pl - 1]
    assert merkle.layer_counts(flens, pl) == ([2, 2, 3, 100], [3, 4, 5, 7])
    for f, c in zip(*reversed(merkle.layer_counts(flens, pl))):
        assert c == len(merkle.file_pieces(flens[f], pl)[0])  # one hash per piece of the file
    assert merkle.layer_counts([], pl) == ([], [])
    with pytest.raises(ValueError):
        merkle.layer_counts([1], pl + 1)


@pytest.mark.parametrize("height", [0, 3])
def test_layer_root_is_the_bep52_model(height):
    from vortex_amd import merkle

    rng = random.Random(7)
    for n in (1, 2, 3, 4, 5, 8, 9, 31, 33, 100):
        rows = [rng.randbytes(32) for _ in range(n)]
        want = model_root(rows, height)
        assert merkle.layer_root(rows, height) == want == merkle.layer_root(b"".join(rows), height)
    with pytest.raises(ValueError):
        merkle.layer_root(b"", height)
    with pytest.raises(ValueError):
        merkle.layer_root(b"x" * 33, height)


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


def test_make_proof_verifies_under_a_plain_walk():
    from vortex_amd import merkle

    rng = random.Random(11)
    height = 3
    for n in (1000, 1024, 5, 1):
        layer = [rng.randbytes(32) for _ in range(n)]
        padded = 1 << (n - 1).bit_length()
        root = model_root(layer, height)
        # every level of the padded tree, for the proofs that stop at an ancestor
        levels = [layer + [_pad(height)] * (padded - n)]
        while len(levels[-1]) > 1:
            lv = levels[-1]
            levels.append([_sha(lv[k], lv[k + 1]) for k in range(0, len(lv), 2)])
        span = 1
        while span <= min(padded, 512):
            total = (padded // span).bit_length() - 1
            for pos in sorted({0, padded // span - 1, (padded // span) // 2, rng.randrange(padded // span)}):
                proof = merkle.make_proof(layer, height, pos, span, total)
                assert len(proof) == 32 * (span + total)
                assert proof[:32 * span] == b"".join(levels[0][pos * span:(pos + 1) * span])
                assert walk(proof, span, total, pos) == root
                half = total // 2
                short = merkle.make_proof(b"".join(layer), height, pos, span, half)
                assert short == proof[:32 * (span + half)]
                assert walk(short, span, half, pos) == levels[span.bit_length() - 1 + half][pos >> half]
                if total and (pos | 1) * span < n:  # a wrong side bit does not verify (where the siblings differ)
                    assert walk(proof, span, total, pos ^ 1) != root
            span *= 2
    # past the layer's own root: the tree goes on with pad hashes
    layer = [rng.randbytes(32) for _ in range(3)]
    proof = merkle.make_proof(layer, 0, 0, 4, 2)
    assert proof[32 * 4:] == _pad(2) + _pad(3)
    assert walk(proof, 4, 2, 0) == model_root(layer + [bytes(32)] * 13, 0)
    with pytest.raises(ValueError):
        merkle.make_proof(layer, 0, 0, 3, 1)


# ---- INTEGRATION.md ------------------------------------------------------------

def test_rust_binding_of_the_new_entries_matches_the_header(monkeypatch):
    """The `extern "C"` lines and `#[repr(C)]` structs INTEGRATION.md gives for
    the new entries, against include/vx_hash.h, with test_integration_doc's
    parsers (that test reads the document's first Rust block only)."""
    import re

    import test_integration_doc as doc

    names = {"u16": "uint16_t", "VxMerkleTile": "vx_merkle_tile", "VxMerkleProof": "vx_merkle_proof",
             "VxMerkleLayersPlan": "vx_merkle_layers_plan"}
    for k, v in names.items():
        monkeypatch.setitem(doc.RUST_TO_C, k, v)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = next(b for b in re.findall(r"```rust\n(.*?)```", text, flags=re.S) if "vx_merkle_verify_layers" in b)
    monkeypatch.setattr(doc, "rust_block", lambda: block)
    rust, c = doc.rust_externs(), doc.c_prototypes()
    assert set(rust) == NEW

    def untagged(t):  # C names the plan by its tag: `struct vx_merkle_layers_plan`, const or not
        return t.replace("structc vx_merkle_layers_plan", "vx_merkle_layers_planc").replace("struct ", "")

    for name, (ret, args) in rust.items():
        cret, cargs = c[name]
        assert ret == cret and args == [untagged(a) for a in cargs], (name, args, cargs)
    structs, cstructs = doc.rust_structs(), doc.c_structs()
    assert structs["VxMerkleTile"] == cstructs["vx_merkle_tile"]
    assert structs["VxMerkleProof"] == cstructs["vx_merkle_proof"]
    # the plan is no typedef, so c_structs does not see it: its fields from the ctypes mirror, checked against C above
    from vortex_amd import _lib

    ctype_names = {ctypes.c_uint32: "uint32_t", ctypes.c_uint64: "uint64_t", ctypes.c_uint32 * 4: "uint32_t[4]"}
    assert structs["VxMerkleLayersPlan"] == [(n, ctype_names[t]) for n, t in _lib.vx_merkle_layers_plan._fields_]
