"""CPU: the v2 download path's ABI (vx_merkle_submit / vx_merkle_poll /
vx_merkle_device_pieces): the completion's C layout against its ctypes mirror,
the symbols in the header, both libraries and _lib.EXPORTS, and the argument
checks that need no device."""
import ctypes
import os
import subprocess

from conftest import ROOT
from test_abi import declared_symbols, dynamic_symbols

NEW = ("vx_merkle_submit", "vx_merkle_poll", "vx_merkle_device_pieces")


def test_merkle_completion_layout(tmp_path):
    """vx_hash.h compiles as C, sizeof(vx_merkle_completion) is 48 and every
    field lies where the ctypes mirror puts it."""
    from vortex_amd._lib import vx_merkle_completion

    fields = [name for name, _ in vx_merkle_completion._fields_]
    assert fields == ["tag", "matched", "root", "_pad"]
    c = tmp_path / "m.c"
    body = ", ".join(f"offsetof(vx_merkle_completion, {f})" for f in fields)
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vx_hash.h"\n'
                 'typedef char size_is_48[sizeof(vx_merkle_completion) == 48 ? 1 : -1];\n'
                 'int main(void){size_t o[] = {' + body + '}; printf("%zu %d", sizeof(vx_merkle_completion), '
                 'VX_ABI_VERSION); for (size_t i = 0; i < sizeof(o) / sizeof(o[0]); ++i) printf(" %zu", o[i]); '
                 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:2] == [48, 3]  # the struct's size; VX_ABI_VERSION stays 3
    assert ctypes.sizeof(vx_merkle_completion) == 48
    assert got[2:] == [getattr(vx_merkle_completion, f).offset for f in fields] == [0, 8, 9, 41]


def test_new_symbols_declared_and_exported(built):
    from vortex_amd import _lib

    decl = declared_symbols()
    for name in NEW:
        assert name in decl, f"{name} is not declared in vx_hash.h"
        assert name in _lib.EXPORTS
        assert name in dynamic_symbols(_lib.LIB_PATH) and name in dynamic_symbols(_lib.TUNING_PATH)
        assert hasattr(_lib.lib(), name) and hasattr(_lib.tuning(), name)
    assert _lib.lib().vx_abi_version() == 3 == _lib.ABI_VERSION == _lib.tuning().vx_abi_version()


def test_integration_doc_binds_the_v2_entries_as_declared():
    """INTEGRATION.md's v2 download snippet against include/vx_hash.h: every
    bound name is declared, with the same arguments and return type, and the
    Rust completion has the C struct's fields."""
    import re

    import test_integration_doc as doc

    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```rust\n(.*?)```", text, flags=re.S) if "vx_merkle_submit" in b]
    assert len(blocks) == 1
    rust_to_c = dict(doc.RUST_TO_C, VxMerkleCompletion="vx_merkle_completion")

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
        assert name in protos, f"{name} is bound in INTEGRATION.md but not declared in include/vx_hash.h"
        assert sig == protos[name], f"{name}: {sig} (Rust) vs {protos[name]} (C)"
    sm = re.search(r"#\[repr\(C\)\]\s*pub struct VxMerkleCompletion\s*\{(.*?)\}", blocks[0], flags=re.S)
    fields = []
    for f in re.split(r",\s*(?![^\[]*\])", sm.group(1)):
        if f.strip():
            fname, t = re.sub(r"^pub\s+", "", f.strip()).split(":", 1)
            fields.append((fname.strip(), to_c(t)))
    want = [(n, t.replace("VX_SHA256_LEN", "32")) for n, t in doc.c_structs()["vx_merkle_completion"]]
    assert fields == want


def test_null_context_and_device_entry_checks(built):
    """Argument errors come back before anything touches a device."""
    from vortex_amd import _lib

    for L in (_lib.lib(), _lib.tuning()):
        data = ctypes.create_string_buffer(16384)
        assert L.vx_merkle_submit(None, 1, data, 16384, 0, None) == _lib.VX_EINVAL
        assert b"NULL context" in L.vx_last_error()
        out = (_lib.vx_merkle_completion * 4)()
        assert L.vx_merkle_poll(None, out, 4) < 0
        vp = ctypes.c_void_p
        ok = dict(base=vp(0x10000), offs=vp(0x20000), lens=vp(0x30000), roots=vp(0x40000), work=vp(0x50000))

        def pieces(base=ok["base"], log2_width=2, work=None, n=4, roots=ok["roots"]):
            return L.vx_merkle_device_pieces(base, ok["offs"], ok["lens"], None, n, log2_width, work, roots, None,
                                             None, None)

        assert pieces(base=vp(0x10008)) == _lib.VX_EINVAL  # misaligned base
        assert b"16-byte aligned" in L.vx_last_error()
        assert pieces(log2_width=18, work=ok["work"]) == _lib.VX_EINVAL
        assert b"log2_width > 17" in L.vx_last_error()
        assert pieces(log2_width=9, work=None) == _lib.VX_EINVAL  # wider than a tile: the tops need d_work
        assert b"d_work" in L.vx_last_error()
        assert pieces(log2_width=9, work=vp(0x50008)) == _lib.VX_EINVAL
        assert pieces(base=None) == _lib.VX_EINVAL
        assert pieces(roots=vp(0x40004)) == _lib.VX_EINVAL
        assert pieces(n=1 << 20, log2_width=12, work=ok["work"]) == _lib.VX_EINVAL  # n << log2_width >= 2^32
        assert pieces(n=0, base=None) == 0  # launches nothing, checks nothing
