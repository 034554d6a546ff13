"""CPU: the re-verify's file-hole scan, piece classification and v2 round
packer with the hole predicate (vortex_amd/csrc/vx_extents.hpp,
vx_merkle_rounds.hpp) against the os.lseek model in
vortex_amd/sparse.py, on sparse files made in tmp_path.

The engine's host code runs in tests/native/extents_dump.cpp, a stand-alone
program built here with ASan + UBSan.  The packer's rounds are replayed with
hashlib in the kernels' place: the roots must be the ones of the files' real
bytes."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from _sparse import NO_HOLES, holes_reported, make_file, write_torrent_range
from conftest import ROOT

BLOCK = 16384
PL = 65536


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("exd") / "extents_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "extents_dump.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, mode, paths, flens, pl, cap, *more):
    out = subprocess.run([str(exe), mode, str(pl), str(cap)] + [str(x) for x in more],
                         input="".join(f"{n} {p}\n" for n, p in zip(flens, paths)), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.rstrip("\n").split("\n")
    files, pieces, rounds = [], [], []
    for ln in lines[:-1]:
        kind, *v = ln.split()
        v = [int(x) for x in v]
        if kind == "F":
            files.append((v[1], []))
            assert v[0] == len(files) - 1
        elif kind == "e":
            files[-1][1].append((v[0], v[1]))
        elif kind == "P":
            assert v[0] == len(pieces)
            pieces.append(bool(v[1]))
        elif kind == "R":
            rounds.append({"data_blocks": v[0], "bytes": v[1], "file_bytes": v[2], "hole_blocks": v[3],
                           "hole_bytes": v[4], "reads": [], "table": [], "nodes": []})
        elif kind == "r":
            rounds[-1]["reads"].append(v)
        elif kind == "t":
            rounds[-1]["table"].append(v)
        else:
            rounds[-1]["nodes"].append(v)
    return files, pieces, rounds, json.loads(lines[-1])


def _torrent(tmp_path, data_seed=7):
    """The v1 layout of the checks: every way a file can lack bytes, with piece
    boundaries that fall inside 4 KiB blocks of the files (the lengths are odd).
    f0 truncated, f1 fallocated, f2 written, f3 one piece written, f4 empty,
    f5 a hole file in front of the written f6, f7 missing, f8 shorter on disk
    (PL / 2, a hole) than its torrent length."""
    import random

    rng = random.Random(data_seed)
    flens = [100_000, 3 * PL + 5, 17, 6 * PL + 1000, 0, 1000, 70_000, 40_000, 2 * PL]
    data = bytes(rng.getrandbits(8) for _ in range(sum(flens)))
    paths = []
    for k, n in enumerate(flens):
        p = tmp_path / f"f{k}"
        if k != 7:
            make_file(p, n, how="fallocate" if k == 1 else "truncate", size=PL // 2 if k == 8 else None)
        paths.append(str(p))
    start = [sum(flens[:k]) for k in range(len(flens))]
    write_torrent_range(paths, flens, start[2], start[2] + 17, data)
    write_torrent_range(paths, flens, start[6], start[6] + flens[6], data)
    k3 = (start[3] + 2 * PL) // PL + 1  # a piece wholly inside f3, not at its edges
    write_torrent_range(paths, flens, k3 * PL, (k3 + 1) * PL, data)
    return paths, flens, start, k3


def test_scan_and_pieces_match_the_model(dump, tmp_path):
    from vortex_amd import sparse

    paths, flens, start, k3 = _torrent(tmp_path)
    files, pieces, _, summary = _run(dump, "v1", paths, flens, PL, sparse.MAX_EXTENTS)
    assert files == [sparse.data_extents(p, n) for p, n in zip(paths, flens)]
    want, extents = sparse.hole_pieces(paths, flens, PL)
    assert pieces == want and summary["extents"] == extents and summary["hole_pieces"] == sum(want)
    n = (sum(flens) + PL - 1) // PL
    assert summary["pieces"] == n == len(pieces)
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    # a truncated and a fallocated file are one hole each; empty, missing: no holes; short: a hole to its size
    assert files[0] == (100_000, []) and files[1] == (3 * PL + 5, []) and files[5] == (1000, [])
    assert files[4] == (0, []) and files[7] == (0, []) and files[8] == (PL // 2, [])
    assert files[2] == (17, [(0, 17)]) and files[6] == (70_000, [(0, 70_000)])

    def piece_of(off):
        return off // PL

    # pieces 0 and 1 lie in f0 and f0 | f1: holes; the piece that holds f2's 17 bytes is not
    assert pieces[0] and pieces[1] and not pieces[piece_of(start[2])]
    # the written piece of f3 and both its unwritten neighbours (the file system keeps whole 4 KiB
    # blocks, and the piece's edges fall inside one) are read; the piece after the next is a hole
    assert not pieces[k3 - 1] and not pieces[k3] and not pieces[k3 + 1] and pieces[k3 + 2]
    # one piece holds f3's unwritten tail, the hole file f5 and the head of the written f6: it is read
    assert piece_of(start[5] - 1) == piece_of(start[5]) == piece_of(start[6]) and not pieces[piece_of(start[6])]
    # nothing of the missing f7, and nothing past the end of the short f8, is a hole
    assert not any(pieces[piece_of(start[6]):])
    assert sum(pieces) == sum(want) > 4


@pytest.mark.parametrize("cap", [1, 3, 8, 100])
def test_extent_cap(dump, tmp_path, cap):
    """Past `cap` extents the rest of the file is data."""
    from vortex_amd import sparse

    n = 8 * PL
    p = make_file(tmp_path / "many", n, writes=[(k * PL + 5, b"x") for k in range(8)])
    files, pieces, _, _ = _run(dump, "v1", [p], [n], PL, cap)
    assert files == [sparse.data_extents(p, n, cap)]
    assert pieces == sparse.hole_pieces([p], [n], PL, cap)[0]
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    bound, ext = files[0]
    assert bound == n and len(ext) == (8 if cap > 8 else cap + 1)  # (after 8 extents the file's last hole follows)
    if cap <= 8:
        assert ext[-1][1] == n and ext[-1][0] == ext[-2][1]  # the tail is one data extent to the bound
    assert not any(pieces)  # every piece holds a written byte


def _v2_root(rows, lw):
    rows = list(rows)
    assert len(rows) == 1 << lw
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


@pytest.mark.parametrize("bpr", [3, 16])
def test_packer_rounds_replayed_with_hashlib(dump, tmp_path, bpr):
    """The rounds the packer makes over sparse files, with hashlib in the
    kernels' place (a hole row is sha256(bytes(l)), an absent slot 32 zero
    bytes): every piece's root is merkle's model over the file's real bytes,
    only written blocks are read, and the hole rows are the model's."""
    import random

    from vortex_amd import hybrid, merkle, sparse

    rng = random.Random(11)
    flens = [3 * PL + 20_000, 20_000, PL + 5_000, 2 * PL, 5 * PL, 16_384 + 1]
    body = [bytes(rng.getrandbits(8) for _ in range(n)) for n in flens]
    paths = [
        # two written blocks and two hole blocks in piece 0, the rest (a short last piece too) holes
        make_file(tmp_path / "a", flens[0], writes=[(BLOCK, body[0][BLOCK:3 * BLOCK])]),
        make_file(tmp_path / "b", flens[1], how="fallocate"),                    # a short file wholly a hole
        make_file(tmp_path / "c", flens[2], writes=[(0, body[2][:PL])]),         # its short last block is a hole
        make_file(tmp_path / "d", flens[3], writes=[(0, body[3])]),              # all data
        make_file(tmp_path / "e", flens[4]),                                     # all hole: five pieces
        make_file(tmp_path / "f", flens[5], writes=[(BLOCK, body[5][BLOCK:])]),  # one hole block, one byte of data
    ]
    # both scans before anything reads the files: a fallocated range that has been read through the
    # page cache reports as data while its pages stay cached
    hb, extents = sparse.hole_blocks(paths, flens, PL)
    _, _, rounds, summary = _run(dump, "v2", paths, flens, PL, sparse.MAX_EXTENTS, 0, -1, bpr)
    real = [open(p, "rb").read() for p in paths]
    lens, log2w, findex, foff = merkle.torrent_pieces(flens, PL)
    want_roots = [hybrid.v2_root(real[f][o:o + n], w) for n, w, f, o in zip(lens, log2w, findex, foff)]
    R = summary["window_rows"]
    ring, roots, read_bytes, hole_lens = {}, {}, 0, []
    for r in rounds:
        stage = bytearray(r["data_blocks"] * BLOCK)
        for file, off, ln, sb, _ in r["reads"]:
            stage[sb * BLOCK:sb * BLOCK + ln] = real[file][off:off + ln]
            read_bytes += ln
        nd, nh = r["data_blocks"], r["hole_blocks"]
        assert len(r["reads"]) == 0 or nd and r["bytes"] <= nd * BLOCK
        table = r["table"]
        for b, (row, ln) in enumerate(table):
            assert 0 <= row < R
            if b < nd:
                assert 0 < ln <= BLOCK
                ring[row] = hashlib.sha256(bytes(stage[b * BLOCK:b * BLOCK + ln])).digest()
            elif b < len(table) - nh:
                assert ln == 0
                ring[row] = bytes(32)
            else:
                assert 0 < ln <= BLOCK
                ring[row] = hashlib.sha256(bytes(ln)).digest()
                hole_lens.append(ln)
        assert r["hole_bytes"] == sum(ln for _, ln in table[len(table) - nh:])
        for g_first, g_n, K, row0 in r["nodes"]:
            for k in range(g_n):
                piece = g_first + k
                base = row0 + (k << K)
                roots[piece] = _v2_root([ring[base + s] for s in range(1 << log2w[piece])], log2w[piece])
    assert [roots[i] for i in range(len(lens))] == want_roots
    model_holes = [min(BLOCK, n - k * BLOCK) for n, blocks in zip(lens, hb) for k, h in enumerate(blocks) if h]
    assert sorted(hole_lens) == sorted(model_holes) and summary["extents"] == extents
    assert summary["hole_bytes"] == sum(model_holes) and read_bytes == sum(flens) - sum(model_holes)
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    assert hb[0] == [True, False, False, True] and all(all(b) for b in hb[1:5])   # file a, then file b
    assert hb[5] == [False] * 4 and hb[6] == [True]                                # file c: data, then its short tail
    assert all(all(b) for b in hb[9:14]) and hb[14] == [True, False]               # e: holes; f: hole, one byte


def test_header_and_exports(built, tmp_path):
    """The new entries are declared for C99, exported by both libraries, and
    check their arguments before anything touches a device."""
    from vortex_amd import _lib

    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "typedef char trace_is_48[sizeof(vx_hole_trace) == 48 ? 1 : -1];\n"
                 "typedef char config_is_56[sizeof(vx_config) == 56 && VX_ABI_VERSION == 3 ? 1 : -1];\n"
                 "int main(void) {\n"
                 "  int (*a)(vx_ctx*, int) = vx_set_skip_holes;\n"
                 "  int (*b)(const vx_ctx*, vx_hole_trace*) = vx_last_verify_holes;\n"
                 "  int (*d)(const uint32_t*, uint32_t, void*, void*) = vx_sha1_device_zeros;\n"
                 "  int (*e)(const uint32_t*, uint32_t, void*, void*) = vx_merkle_device_zero_leaves;\n"
                 "  (void)a; (void)b; (void)d; (void)e; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o",
                    str(tmp_path / "t.o")], check=True)
    assert ctypes.sizeof(_lib.vx_hole_trace) == 48
    assert [n for n, _ in _lib.vx_hole_trace._fields_] == ["hole_pieces", "hole_blocks", "hole_bytes", "extents",
                                                           "scan_ms", "zero_hash_ms"]
    for L in (_lib.lib(), _lib.tuning()):
        t = _lib.vx_hole_trace()
        assert L.vx_set_skip_holes(None, 1) == _lib.VX_EINVAL and b"vx_set_skip_holes" in L.vx_last_error()
        assert L.vx_last_verify_holes(None, ctypes.byref(t)) == _lib.VX_EINVAL
        assert L.vx_sha1_device_zeros(None, 0, None, None) == 0            # n == 0 launches nothing
        assert L.vx_sha1_device_zeros(None, 4, None, None) == _lib.VX_EINVAL
        assert L.vx_sha1_device_zeros(ctypes.c_void_p(0x1002), 4, ctypes.c_void_p(0x2000), None) == _lib.VX_EINVAL
        assert L.vx_merkle_device_zero_leaves(None, 0, None, None) == 0
        assert L.vx_merkle_device_zero_leaves(None, 4, None, None) == _lib.VX_EINVAL
        assert L.vx_merkle_device_zero_leaves(ctypes.c_void_p(0x1000), 4, ctypes.c_void_p(0x2008),
                                              None) == _lib.VX_EINVAL
        assert b"aligned" in L.vx_last_error()
