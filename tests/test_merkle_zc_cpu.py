"""CPU: the zero-copy v2 download path's host side (vx_set_merkle_zero_copy,
vx_merkle_zero_copy_trace, vx_tuning_merkle_zc_geometry) and the sweep that
tests/test_gpu_merkle_zc_sweep.py runs: argument checks without a GPU, the
trace's layout against the header, the kernel's geometry, and that the sweep's
shapes, built from that geometry, reach every class of tests/_merkle_zc_sweep.py.
"""
import ctypes
import os
import subprocess

import _merkle_zc_sweep as zs
from conftest import ROOT


def test_setter_and_trace_validate_without_gpu(built):
    from vortex_amd import _lib

    L = _lib.lib()
    for on in (0, 1, 2, -1):
        assert L.vx_set_merkle_zero_copy(None, on) == _lib.VX_EINVAL
        assert b"vx_set_merkle_zero_copy" in L.vx_last_error()
    t = _lib.merkle_zc_trace_type()()
    assert L.vx_merkle_zero_copy_trace(None, ctypes.byref(t)) == _lib.VX_EINVAL
    assert b"vx_merkle_zero_copy_trace" in L.vx_last_error()
    assert L.vx_merkle_zero_copy_trace(None, None) == _lib.VX_EINVAL
    assert [getattr(t, f) for f in _lib.MERKLE_ZC_TRACE_FIELDS] == [0, 0, 0, 0]
    assert L.vx_abi_version() == 3  # the two calls are additions to ABI 3
    # the kernel's tuning entry refuses its arguments before anything touches a device
    T = _lib.tuning()
    fn = T.vx_tuning_merkle_zc_kernel
    p = ctypes.c_void_p
    assert fn(None, None, None, 0, 3, None, None, None, None) == 0  # n = 0 is a no-op
    assert fn(None, p(0x1000), None, 4, 3, p(0x2000), None, None, None) == _lib.VX_EINVAL
    assert fn(p(0x1000), None, None, 4, 3, p(0x2000), None, None, None) == _lib.VX_EINVAL
    assert fn(p(0x1004), p(0x1000), None, 4, 3, p(0x2000), None, None, None) == _lib.VX_EINVAL  # d_srcs: 8 bytes
    assert fn(p(0x1000), p(0x1002), None, 4, 3, p(0x2000), None, None, None) == _lib.VX_EINVAL  # d_lens: 4 bytes
    assert fn(p(0x1000), p(0x1000), None, 4, 18, p(0x2000), None, None, None) == _lib.VX_EINVAL  # width > 17
    assert fn(p(0x1000), p(0x1000), None, 1 << 20, 12, p(0x2000), None, None, None) == _lib.VX_EINVAL  # 2^32 rows
    assert fn(p(0x1000), p(0x1000), None, 4, 3, p(0x2008), None, None, None) == _lib.VX_EINVAL  # d_roots: 16 bytes
    assert b"vx_tuning_merkle_zc_kernel" in T.vx_last_error()


def test_trace_has_the_c_layout(tmp_path):
    """vx_merkle_zc_trace has no struct tag in the header (only its typedef), so
    the binding's structure is checked here: sizeof and every field's offset and
    size, C's against ctypes'."""
    from vortex_amd import _lib

    cls = _lib.merkle_zc_trace_type()
    fields = [f for f, _ in cls._fields_]
    assert tuple(fields) == _lib.MERKLE_ZC_TRACE_FIELDS == ("slots", "pieces", "bytes", "fallback_slots")
    body = 'printf("%zu", sizeof(vx_merkle_zc_trace));' + "".join(
        f'printf(" %zu %zu", offsetof(vx_merkle_zc_trace, {f}), sizeof(((vx_merkle_zc_trace*)0)->{f}));'
        for f in fields)
    c = tmp_path / "t.c"
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vx_hash.h"\n'
                 "int main(void) {" + body + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "t"
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    subprocess.run(gcc + [str(c), "-o", str(exe)], check=True)
    nums = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    # ... and the two prototypes are the issue's (compiled, not linked)
    p = tmp_path / "p.c"
    p.write_text('#include "vx_hash.h"\nint (*set_fn)(vx_ctx*, int) = vx_set_merkle_zero_copy;\n'
                 "int (*trace_fn)(const vx_ctx*, vx_merkle_zc_trace*) = vx_merkle_zero_copy_trace;\n")
    subprocess.run(gcc + ["-c", str(p), "-o", str(tmp_path / "p.o")], check=True)
    want = [ctypes.sizeof(cls)]
    for f in fields:
        want += [getattr(cls, f).offset, getattr(cls, f).size]
    assert nums == want == [32, 0, 8, 8, 8, 16, 8, 24, 8]


def test_geometry(built):
    geo = zs.geometry()
    for v in geo:
        assert v >= 1 and v & (v - 1) == 0, geo  # powers of two
    assert geo.group == 256  # a workgroup keeps 256 leaf rows: the tree phase is merkle_piece_kernel's
    assert geo.wave <= geo.group and geo.tile % 16 == 0 and geo.tile <= zs.LEAF
    assert zs.lds_bytes(geo) <= 160 * 1024
    # the shape DESIGN.md §6.5 measured: 16 lanes x 16 bytes on each of 4 sources per wave instruction
    assert geo.tile == 256 and 64 // (geo.tile // 16) == 4


def test_sweep_reaches_every_class(built):
    geo = zs.geometry()
    T, F = geo.tile, geo.inflight
    for W in (1, 2, 1024):
        ls = zs.lengths(geo, W)
        for v in (0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1,
                  16383, 16384, W * zs.LEAF - 1, W * zs.LEAF):
            assert v in ls, (W, v)
        assert (16385 in ls) == (W > 1)
        tiles = {v // T for v in ls if v <= zs.LEAF}
        assert any(t % 2 for t in tiles if t) and any(t % 2 == 0 for t in tiles if t)
        assert any(t and t % F == 0 for t in tiles) and any(t > F and t % F == 1 for t in tiles)
    runs = zs.launches(geo)
    assert len({r.name for r in runs}) == len(runs)
    got, src = set(), set()
    for r in runs:
        assert all(v <= zs.LEAF << lw and lw <= r.K for v, lw in r.pieces), r.name
        got |= zs.classes(geo, r)
        buf, offs = zs.place(r)
        src |= zs.source_classes(offs, r.pieces)
        assert all(o % 16 == 0 for o in offs)
        # nothing but FILL outside the pieces: a lane that hashed past an end would get a wrong root
        mask = buf == zs.FILL
        for o, (v, _) in zip(offs, r.pieces):
            mask[o:o + v] = True
        assert mask.all(), r.name
    assert not zs.REQUIRED - got, sorted(zs.REQUIRED - got)
    assert src == {"unordered", "aligned16_not256", "gaps"}
    assert sum(v for r in runs for v, _ in r.pieces) < 96 << 20  # the sweep stays small


def test_model_is_the_layer_root_of_the_leaves():
    """The model of the sweep (hybrid.v2_root) against merkle.layer_root over the
    hashlib leaves, for a piece that fills its tree and one that does not."""
    import hashlib

    from vortex_amd import hybrid, merkle

    data = bytes(range(256)) * 300  # 76,800 bytes: 4 full leaves and 11,264 bytes
    full = data[:4 * zs.LEAF]
    leaves = b"".join(hashlib.sha256(full[o:o + zs.LEAF]).digest() for o in range(0, len(full), zs.LEAF))
    assert hybrid.v2_root(full, 2) == merkle.layer_root(leaves, 0)
    rows = [hashlib.sha256(data[o:o + zs.LEAF]).digest() for o in range(0, len(data), zs.LEAF)]
    assert hybrid.v2_root(data, 3) == merkle.layer_root(b"".join(rows), 0)  # 5 leaves in a tree of 8: zero rows
