"""The Python binding's types must be the headers'.

vortex_amd/_lib.py declares every function's argtypes and restype by hand, and
every GPU test calls through those tables.  A c_uint32 where the header says
uint64_t is harmless in the first six integer arguments on x86-64; from the
seventh on the value goes to the stack, libffi writes only the declared width
into the 8-byte slot, and the upper half is whatever was there: an intermittent
wrong row count, not a failing test.  So this test parses every prototype of
include/vx_hash.h, vx_tuning.h and vx_synth.h (with the parser that checks
INTEGRATION.md's Rust binding, tests/test_integration_doc.py), lets
_lib._declare fill a stand-in object (no built library is needed), and compares
the two function by function; and it compares every ctypes.Structure of _lib.py
that has a C namesake with the C struct's size and field offsets, from one
small C program compiled from the headers.  CPU only.
"""
import copy
import ctypes
import os
import re
import subprocess
import types

import pytest

from conftest import ROOT
from test_integration_doc import c_prototypes

HEADERS = ("vx_hash.h", "vx_tuning.h", "vx_synth.h")
# a value type of the headers -> (kind, bits); anything else fails the test, so the table stays complete
C_VALUES = {"int": ("int", 32), "int32_t": ("int", 32), "uint32_t": ("uint", 32), "uint64_t": ("uint", 64),
            "size_t": ("uint", 64), "int64_t": ("int", 64), "double": ("double", 64), "void": ("void", 0)}
CT_CODES = {"i": "int", "l": "int", "q": "int", "I": "uint", "L": "uint", "Q": "uint", "d": "double"}


def c_kind(t):
    """A header type in norm_c's form -> ("pointer", 0) or (kind, bits)."""
    if t.endswith("*"):
        return ("pointer", 0)
    base = t[:-1] if t.endswith("c") and t[:-1] in C_VALUES else t
    if base not in C_VALUES:
        raise KeyError(f"test_binding_cpu.C_VALUES has no entry for the header's type `{t}`")
    return C_VALUES[base]


def ct_kind(t):
    """A ctypes type of the binding -> the same."""
    if t is None:
        return ("void", 0)
    if isinstance(t, type) and issubclass(t, (ctypes._Pointer, ctypes.Array)) or t in (ctypes.c_void_p, ctypes.c_char_p):
        return ("pointer", 0)
    if isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t._type_ in CT_CODES:
        return (CT_CODES[t._type_], 8 * ctypes.sizeof(t))
    raise KeyError(f"test_binding_cpu.ct_kind cannot place the binding's type {t!r}")


class Recorder:
    """Stands in for the CDLL: _declare sets argtypes and restype on its attributes."""

    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.fns.setdefault(name, types.SimpleNamespace())


def declared(tuning=True):
    """{name: (argtypes, restype)} as _lib._declare sets them."""
    from vortex_amd import _lib

    rec = Recorder()
    _lib._declare(rec, tuning)
    return {name: (list(fn.argtypes), fn.restype) for name, fn in rec.fns.items()}


def show(kind):
    return kind[0] if kind[0] in ("pointer", "void") else f"{kind[0]}{kind[1]}"


def compare(protos, table):
    """Every difference between the headers' prototypes and the binding's
    table, as "function: what" lines; arguments count from 1."""
    problems = []
    for name in sorted(set(protos) | set(table)):
        if name not in table:
            problems.append(f"{name}: declared in the headers, not in _lib._declare")
            continue
        if name not in protos:
            problems.append(f"{name}: declared in _lib._declare, not in the headers")
            continue
        (cret, cargs), (pargs, pret) = protos[name], table[name]
        if len(cargs) != len(pargs):
            problems.append(f"{name}: {len(pargs)} arguments in _lib.py, {len(cargs)} in the header")
        else:
            for k, (c, p) in enumerate(zip(cargs, pargs), 1):
                if c_kind(c) != ct_kind(p):
                    problems.append(f"{name}: argument {k} is {show(ct_kind(p))} in _lib.py, "
                                    f"{show(c_kind(c))} (`{c}`) in the header")
        if c_kind(cret) != ct_kind(pret):
            problems.append(f"{name}: returns {show(ct_kind(pret))} in _lib.py, {show(c_kind(cret))} (`{cret}`) "
                            "in the header")
    return problems


def test_parser_reads_every_prototype():
    """The parse is the export lists': nothing the headers declare is skipped."""
    from vortex_amd import _lib

    assert set(c_prototypes(("vx_hash.h",))) == set(_lib.EXPORTS)
    assert set(c_prototypes(HEADERS)) == set(_lib.EXPORTS) | set(_lib.TUNING_EXPORTS)
    protos = c_prototypes(HEADERS)
    assert protos["vx_merkle_hash_files_leaves"][1][9] == protos["vx_merkle_hash_files_leaves"][1][11] == "uint64_t"
    assert len(protos["vx_merkle_hash_files_leaves"][1]) == 13 and protos["vx_last_error"] == ("charc *", [])
    assert protos["vx_tuning_zero_leaf_kernel"] == ("int", ["uint32_tc *", "uint32_tc *", "uint32_t", "void *",
                                                            "voidc *", "void *"])
    assert protos["vx_tuning_gather_kernel"] == ("int", ["uint64_tc *", "uint64_tc *", "uint32_tc *", "uint32_tc *",
                                                         "uint32_t", "uint32_t", "void *", "uint32_t", "void *"])


def test_binding_matches_the_headers():
    from vortex_amd import _lib

    table = declared(tuning=True)
    assert not compare(c_prototypes(HEADERS), table), "\n".join(compare(c_prototypes(HEADERS), table))
    release = declared(tuning=False)
    assert set(release) == set(_lib.EXPORTS) and all(table[name] == release[name] for name in release)
    kinds = {ct_kind(t) for args, res in table.values() for t in args + [res]}
    assert kinds == {("pointer", 0), ("void", 0), ("int", 32), ("uint", 32), ("int", 64), ("uint", 64), ("double", 64)}


def _narrow(table):
    args = table["vx_merkle_hash_files_leaves"][0]
    assert args[9] is ctypes.c_uint64
    args[9] = ctypes.c_uint32


def _drop(table):
    del table["vx_tuning_hybrid_finish_kernel"][0][5]


def _swap(table):
    args = table["vx_sha1_device_zeros"][0]
    args[0], args[1] = args[1], args[0]


def _int_return(table):
    args, res = table["vx_merkle_verify_files_blocks"]
    assert res is ctypes.c_int64
    table["vx_merkle_verify_files_blocks"] = (args, ctypes.c_int)


def _signed(table):
    table["vx_merkle_tree_proof"][0][4] = ctypes.c_int64


def _undeclared(table):
    del table["vx_tuning_zero_leaf_kernel"]


def _gather_grid_as_pointer(table):
    args = table["vx_tuning_gather_kernel"][0]
    assert args[7] is ctypes.c_uint32  # the eighth argument goes to the stack: its width counts
    args[7] = ctypes.c_void_p


@pytest.mark.parametrize("doctor,needles", [
    (_narrow, ["vx_merkle_hash_files_leaves: argument 10 is uint32 in _lib.py, uint64 (`uint64_t`) in the header"]),
    (_drop, ["vx_tuning_hybrid_finish_kernel: 14 arguments in _lib.py, 15 in the header"]),
    (_swap, ["vx_sha1_device_zeros: argument 1 is uint32 in _lib.py, pointer (`uint32_tc *`) in the header",
             "vx_sha1_device_zeros: argument 2 is pointer in _lib.py, uint32 (`uint32_t`) in the header"]),
    (_int_return, ["vx_merkle_verify_files_blocks: returns int32 in _lib.py, int64 (`int64_t`) in the header"]),
    (_signed, ["vx_merkle_tree_proof: argument 5 is int64 in _lib.py, uint64 (`uint64_t`) in the header"]),
    (_undeclared, ["vx_tuning_zero_leaf_kernel: declared in the headers, not in _lib._declare"]),
    (_gather_grid_as_pointer, ["vx_tuning_gather_kernel: argument 8 is pointer in _lib.py, uint32 (`uint32_t`) in "
                               "the header"]),
])
def test_checker_rejects_known_mistakes(doctor, needles):
    """The comparison bites: each doctored table is reported by function name
    and argument position, and nothing else is."""
    table = {name: (list(args), res) for name, (args, res) in declared().items()}
    doctor(table)
    assert compare(c_prototypes(HEADERS), table) == needles


def test_checker_rejects_an_unknown_header_type():
    protos = copy.deepcopy(c_prototypes(HEADERS))
    protos["vx_pending"][1][0] = "long"
    with pytest.raises(KeyError, match="no entry for the header's type `long`"):
        compare(protos, declared())


# ---------------------------------------------------------------------------
# Structures
# ---------------------------------------------------------------------------
def c_struct_names():
    text = "\n".join(open(os.path.join(ROOT, "include", h)).read() for h in HEADERS)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\bstruct\s+(\w+)\s*\{", text))


def binding_structs():
    from vortex_amd import _lib

    return {name: cls for name, cls in vars(_lib).items()
            if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure}


def test_every_structure_has_the_c_layout(tmp_path):
    """sizeof and every field's offset and size, C's against ctypes', for every
    Structure of _lib.py with a C namesake, which is every one of them."""
    structs = binding_structs()
    assert set(structs) == c_struct_names() and len(structs) == 15
    lines = []
    for name, cls in sorted(structs.items()):
        fields = [f for f, *_ in cls._fields_]
        lines.append(f'printf("{name} %zu", sizeof(struct {name}));')
        lines += [f'printf(" %zu %zu", offsetof(struct {name}, {f}), sizeof(((struct {name}*)0)->{f}));' for f in fields]
        lines.append('printf("\\n");')
    c = tmp_path / "layout.c"
    c.write_text("#include <stddef.h>\n#include <stdio.h>\n" + "".join(f'#include "{h}"\n' for h in HEADERS)
                 + "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(structs)
    for line in out:
        name, *nums = line.split()
        cls = structs[name]
        want = [ctypes.sizeof(cls)]
        for f, *_ in cls._fields_:
            want += [getattr(cls, f).offset, getattr(cls, f).size]
        assert list(map(int, nums)) == want, f"{name}: C has (sizeof, then offset and size of each field) {nums}, ctypes {want}"
