"""CPU: the hybrid download path's ABI (vx_hybrid_submit / _set_piece_tables /
_submit_piece / _poll): the completion's C layout against its ctypes mirror,
the symbols in the header, both libraries and _lib.EXPORTS, INTEGRATION.md's
binding, the checks that need no device, and the host-only part of a hybrid
slot (vortex_amd/csrc/vx_hybrid_slot.hpp: the argument check, the lane values
and the packed metadata layout) run as a stand-alone program under ASan + UBSan
against a Python model."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_abi import declared_symbols, dynamic_symbols

NEW = ("vx_hybrid_submit", "vx_hybrid_set_piece_tables", "vx_hybrid_submit_piece", "vx_hybrid_poll")
BLOCK = 16384
VX_EINVAL, VX_ERANGE = -22, -34


def test_hybrid_completion_layout(tmp_path):
    """vx_hash.h compiles as C, sizeof(vx_hybrid_completion) is 64 and every
    field lies where the issue and the ctypes mirror put it."""
    from vortex_amd._lib import vx_hybrid_completion

    fields = [name for name, _ in vx_hybrid_completion._fields_]
    assert fields == ["tag", "matched", "_pad", "sha1", "root"]
    c = tmp_path / "h.c"
    body = ", ".join(f"offsetof(vx_hybrid_completion, {f})" for f in fields)
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vx_hash.h"\n'
                 'typedef char size_is_64[sizeof(vx_hybrid_completion) == 64 ? 1 : -1];\n'
                 'int main(void){size_t o[] = {' + body + '}; printf("%zu %d", sizeof(vx_hybrid_completion), '
                 'VX_ABI_VERSION); for (size_t i = 0; i < sizeof(o) / sizeof(o[0]); ++i) printf(" %zu", o[i]); '
                 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "h"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:2] == [64, 3]  # the struct's size; VX_ABI_VERSION stays 3
    assert ctypes.sizeof(vx_hybrid_completion) == 64
    assert got[2:] == [getattr(vx_hybrid_completion, f).offset for f in fields] == [0, 8, 9, 12, 32]


def test_new_symbols_declared_and_exported(built):
    from vortex_amd import _lib

    decl = declared_symbols()
    for name in NEW:
        assert name in decl, f"{name} is not declared in vx_hash.h"
        assert name in _lib.EXPORTS
        assert name in dynamic_symbols(_lib.LIB_PATH) and name in dynamic_symbols(_lib.TUNING_PATH)
        assert getattr(_lib.lib(), name).argtypes is not None and getattr(_lib.tuning(), name).argtypes is not None
    assert _lib.lib().vx_hybrid_poll.restype is ctypes.c_int64
    assert _lib.lib().vx_abi_version() == 3 == _lib.ABI_VERSION == _lib.tuning().vx_abi_version()


def test_integration_doc_binds_the_hybrid_entries_as_declared():
    """INTEGRATION.md's hybrid download snippet against include/vx_hash.h: every
    new entry is bound, with the declared arguments and return type, and the
    Rust completion has the C struct's fields."""
    import test_integration_doc as doc

    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```rust\n(.*?)```", text, flags=re.S) if "fn vx_hybrid_submit(" in b]
    assert len(blocks) == 1
    rust_to_c = dict(doc.RUST_TO_C, VxHybridCompletion="vx_hybrid_completion")

    def to_c(t):
        t = t.strip()
        m = re.fullmatch(r"\[(\w+);\s*(\d+)\]", t)
        if m:
            return f"{to_c(m.group(1))}[{m.group(2)}]"
        m = re.fullmatch(r"\*(const|mut)\s+(.+)", t)
        if m:
            inner = to_c(m.group(2)).split(" ")
            if m.group(1) == "const":
                inner[-1] += "c"
            return " ".join(inner + ["*"])
        return rust_to_c[t]

    protos = doc.c_prototypes()
    bound = {}
    ext = re.search(r'extern "C" \{(.*?)\n\}', blocks[0], flags=re.S).group(1)
    for m in re.finditer(r"fn (vx_\w+)\((.*?)\)\s*->\s*(\w+)\s*;", ext, flags=re.S):
        bound[m.group(1)] = (rust_to_c[m.group(3)], [to_c(a.split(":", 1)[1]) for a in m.group(2).split(",")])
    assert set(bound) == set(NEW)
    for name, sig in bound.items():
        assert sig == protos[name], f"{name}: {sig} (Rust) vs {protos[name]} (C)"
    sm = re.search(r"#\[repr\(C\)\]\s*pub struct VxHybridCompletion\s*\{(.*?)\}", blocks[0], flags=re.S)
    fields = []
    for f in re.split(r",\s*(?![^\[]*\])", sm.group(1)):
        if f.strip():
            fname, t = re.sub(r"^pub\s+", "", f.strip()).split(":", 1)
            fields.append((fname.strip(), to_c(t)))
    want = [(n, t.replace("VX_SHA256_LEN", "32")) for n, t in doc.c_structs()["vx_hybrid_completion"]]
    assert fields == want
    # the call-site sketch behind the binding uses the entries it binds
    for name in ("vx_hybrid_set_piece_tables(ctx", "vx_hybrid_submit_piece(ctx", "vx_hybrid_poll(ctx"):
        assert name in text


def test_null_context_returns_einval(built):
    from vortex_amd import _lib

    for L in (_lib.lib(), _lib.tuning()):
        data = ctypes.create_string_buffer(16384)
        assert L.vx_hybrid_submit(None, 1, data, 16384, 0, 0, None, None) == _lib.VX_EINVAL
        assert b"NULL context" in L.vx_last_error()
        assert L.vx_hybrid_submit_piece(None, 1, data, 16384, 0, 0, 0) == _lib.VX_EINVAL
        assert b"NULL context" in L.vx_last_error()
        assert L.vx_hybrid_set_piece_tables(None, data, data, 1) == _lib.VX_EINVAL
        out = (_lib.vx_hybrid_completion * 4)()
        assert L.vx_hybrid_poll(None, out, 4) == _lib.VX_EINVAL


def test_python_argument_checks_raise_before_the_library(built):
    """ValueError for 20- / 32-byte rows, the buffer size and the uint32 ranges,
    on a pool whose library would crash if it were reached (no context)."""
    from vortex_amd import _lib
    from vortex_amd.hash_pool import DownloadedHybridPiece, HashPool

    class Unreachable:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached: {name}")

    pool = HashPool.__new__(HashPool)
    pool.lib, pool._h, pool._hybrid_rows, pool._next_tag, pool._inflight = Unreachable(), None, 8, 0, {}
    pool.config = _lib.vx_config()
    pool.config.max_piece_len = 65536
    buf = bytearray(65536)
    for kw in (dict(expected_sha1=b"x" * 19), dict(expected_sha1=b"x" * 32), dict(expected_root=b"y" * 20),
               dict(expected_root=b"y" * 33), dict(pad_len=-1), dict(pad_len=1 << 32), dict(log2w=-1),
               dict(log2w=1 << 32)):
        with pytest.raises(ValueError):
            pool.spawn_hybrid(0, 0, buf, 1000, **kw)
    with pytest.raises(ValueError):
        pool.spawn_hybrid(0, 0, buf, 65537)  # piece_len exceeds the buffer
    with pytest.raises(ValueError):
        pool.spawn_hybrid(0, 0, buf, -1)
    with pytest.raises(ValueError):
        pool.spawn_hybrid(1 << 32, 0, buf, 1000)  # by index: a row number is a uint32
    for pieces, roots in ((b"a" * 21, b"b" * 32), (b"a" * 20, b"b" * 33), (b"a" * 40, b"b" * 32), (b"", b"b" * 32)):
        with pytest.raises(ValueError):
            pool.set_hybrid_tables(pieces, roots)
    assert pool._inflight == {} and pool._next_tag == 0
    pool._h = None  # (nothing to destroy)
    r = DownloadedHybridPiece(1, 2, 3, None, b"s", b"r")
    assert r.hash_matched and not DownloadedHybridPiece(1, 2, 1, None).hash_matched
    assert not DownloadedHybridPiece(1, 2, 2, None).hash_matched and not DownloadedHybridPiece(1, 2, 0, None).hash_matched


# ---- vx_hybrid_slot.hpp as a stand-alone program --------------------------------

@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("hsd") / "hybrid_slot_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "hybrid_slot_dump.cpp"), "-o", str(exe)], check=True)
    return exe


def model_check(length, pad, log2w, mpl):
    """The issue's argument checks, in vx_merkle_submit's order."""
    widest = BLOCK
    while widest < mpl:
        widest <<= 1
    if length > mpl:
        return VX_ERANGE
    if log2w > 17 or length > BLOCK << log2w or BLOCK << log2w > widest:
        return VX_EINVAL
    if pad == 0:
        return 0
    total = length + pad
    ok = length > 0 and total & (total - 1) == 0 and total >= BLOCK and total >= BLOCK << log2w and total <= widest
    return 0 if ok else VX_EINVAL


def model_lane(off, length, pad, flags):
    """chunk, total, tail offset, zero blocks, mixed: what the chunked kernel
    and the finish kernel take for one piece, from the v1 message's blocks."""
    whole = length // 64 * 64
    chunk = whole if pad else length
    mixed = 1 if pad and length % 64 else 0
    # the message is (length + pad) bytes: its 64-byte blocks are the whole data blocks, the mixed one, zero ones
    zero_blocks = (length + pad) // 64 - whole // 64 - mixed if pad else 0
    return [chunk, length + pad, off + whole, zero_blocks, mixed, flags]


def run_dump(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [ln.split() for ln in out.stdout.strip().split("\n")]


def test_slot_lanes_and_rejections_against_the_model(dump_exe):
    cases = []
    for pl in (16 * 1024, 64 * 1024, 8 << 20):
        lw = (pl // BLOCK).bit_length() - 1
        for length in (0, 1, 55, 56, 63, 64, 65, 16383, 16384, 16385, pl - 1, pl):
            # (16385 at 16 KiB pieces is longer than the piece: VX_ERANGE, and no pad to cross it with)
            for pad in sorted({0, pl - length}) if length <= pl else (0,):
                cases.append((pl, 256 * len(cases), length, pad, lw, len(cases) % 4))
    pl = 64 * 1024
    rejected = [(pl, 0, 0, pl, 2, 3),              # pad with len == 0
                (pl, 0, 1000, pl - 1001, 2, 3),    # total not a power of two
                (pl, 0, 1000, pl + 1 - 1000, 2, 3),
                (pl, 0, 1000, 32768 - 1000, 2, 3),  # total below the tree
                (pl, 0, 1000, 8192 - 1000, 0, 3),   # total a power of two below one block
                (pl, 0, 1000, 2 * pl - 1000, 2, 3),  # total above max_piece_len
                (pl, 0, 1000, 0, 18, 3),           # log2w 18
                (pl, 0, 16385, 0, 0, 3),           # len above the tree
                (pl, 0, 40000, pl - 40000, 1, 3),  # len above the tree, padded
                (pl, 0, 1000, 0, 3, 3),            # tree wider than max_piece_len
                (pl, 0, pl + 1, 0, 3, 3)]          # VX_ERANGE comes first
    got = run_dump(dump_exe, ["L " + " ".join(map(str, c)) for c in cases + rejected])
    assert len(got) == len(cases) + len(rejected)
    accepted = 0
    for c, g in zip(cases + rejected, got):
        mpl, off, length, pad, lw, flags = c
        rc = model_check(length, pad, lw, mpl)
        assert g[0] == "L" and int(g[1]) == rc, (c, g)
        if rc == 0:
            accepted += 1
            assert list(map(int, g[2:])) == model_lane(off, length, pad, flags), (c, g)
        else:
            assert len(g) == 2
    assert [int(g[1]) for g in got[len(cases):]] == [VX_EINVAL] * 10 + [VX_ERANGE]
    # of the crossed cases: len 0 with a pad, and len 16385 at 16 KiB pieces, are the rejected ones
    assert accepted == len(cases) - 3 - 1
    # the properties the kernels rely on, whatever the model says
    for c, g in zip(cases, got):
        if int(g[1]) == 0 and c[3]:
            chunk, total, tail_off, zb, mixed = map(int, g[2:7])
            assert chunk % 64 == 0 and total % 64 == 0 and tail_off % 4 == 0
            assert chunk + 64 * mixed + 64 * zb == total  # every block of the message is hashed once


def test_pack_layout(dump_exe):
    """The one metadata block of a launch: columns in order, 16-byte aligned,
    each large enough for n entries, the states device-only behind the copy."""
    sizes = [8, 8, 8, 8, 8, 4, 4, 4, 4, 4, None, 20, 32, 1, 1]
    for n, g in zip((1, 2, 3, 16, 17, 1000, 65536), run_dump(dump_exe, [f"P {n}" for n in (1, 2, 3, 16, 17, 1000, 65536)])):
        assert g[0] == "P"
        v = list(map(int, g[1:]))
        cols, copy_bytes, states, total = v[:15], v[15], v[16], v[17]
        assert all(o % 16 == 0 for o in cols + [copy_bytes, states, total]) and cols[0] == 0
        ends = cols[1:] + [copy_bytes]
        for o, e, sz in zip(cols, ends, sizes):
            need = n * sz if sz else 4 * (n + 1)
            assert o + need <= e < o + need + 16
        assert states == copy_bytes and total >= states + 20 * n
