"""CPU: hybrid (v1 + v2) torrents — the geometry model (vortex_amd/hybrid.py) and
its numbering proof against a materialised v1 byte stream, the three new C ABI
entries (header, exports, argument validation), and the round planner
(vortex_amd/csrc/vx_hybrid_rounds.hpp) run as a stand-alone program under
ASan+UBSan and replayed in Python: the replay stages the reads, feeds the lanes
and table entries to hashlib as the kernels would take them, and must arrive at
hashlib's digests and roots of the model.  No GPU, no compute calls."""
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

BLOCK = 16384
NEW = {"vx_hybrid_device_pieces", "vx_hybrid_verify_files", "vx_hybrid_verify_files_range"}


def layouts():
    """(name, piece_length, file_lengths): the layouts of the files call's tests."""
    k, m = 65536, 1 << 20
    return [
        ("one-file", k, [2 * k + k // 2 + 17]),
        ("three-files", k, [1, k, k + 1]),
        ("empty-middle", k, [k + 5, 0, 3]),
        ("200-small", k, [100] * 200),
        ("1MiB", m, [2 * m + m // 2 + 17, 300 * 1024, m]),
    ]


def file_bytes(seed, flens):
    rng = random.Random(seed)
    return [rng.randbytes(n) for n in flens]


# ---- geometry ---------------------------------------------------------------

@pytest.mark.parametrize("name,pl,flens", layouts(), ids=[x[0] for x in layouts()])
def test_v1_piece_numbering_equals_v2(name, pl, flens):
    """Cut the v1 byte stream file | pad | file | pad | ... | last file at
    piece_length: piece i is data_i followed by pad_i zeros."""
    from vortex_amd import hybrid, merkle

    files = file_bytes(7, flens)
    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(flens, pl)
    lens2, lw2, fi2, fo2 = merkle.torrent_pieces(flens, pl)
    assert (dlen, log2w, findex, foff) == (lens2, lw2, fi2, fo2)
    last_file = max(f for f, n in enumerate(flens) if n)
    stream = bytearray()
    for f, body in enumerate(files):
        stream += body
        if f != last_file and len(body) % pl:  # BEP 47: a pad file after every file but the last
            stream += bytes(pl - len(body) % pl)
    cut = [bytes(stream[o:o + pl]) for o in range(0, len(stream), pl)]
    assert len(cut) == len(dlen)
    for i, piece in enumerate(cut):
        data = files[findex[i]][foff[i]:foff[i] + dlen[i]]
        assert piece == data + bytes(pads[i]), i
        assert hybrid.v1_digest(data, pads[i]) == hashlib.sha1(piece).digest()
        assert pads[i] in (0, pl - dlen[i])
    assert pads[-1] == 0
    assert sum(dlen) == sum(flens)


def test_geometry_edges():
    from vortex_amd import hybrid

    assert hybrid.hybrid_pieces([], 16384) == ([], [], [], [], [])
    assert hybrid.hybrid_pieces([0, 0], 16384) == ([], [], [], [], [])
    # the last non-empty file is not padded even when empty files follow it
    assert hybrid.hybrid_pieces([5, 7, 0], 16384)[3] == [16384 - 5, 0]
    assert hybrid.hybrid_pieces([16384, 16384], 16384)[3] == [0, 0]
    for bad in (8192, 3 * 16384, 16385, 0):
        with pytest.raises(ValueError):
            hybrid.hybrid_pieces([1], bad)
    with pytest.raises(ValueError):
        hybrid.v1_digest(b"x", -1)
    assert hybrid.v1_digest(b"abc", 3 << 20) == hashlib.sha1(b"abc" + bytes(3 << 20)).digest()


# ---- the C ABI ----------------------------------------------------------------

def test_header_declares_the_new_entries_as_c99(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "vx_hash.h"\n'
                 "int main(void){\n"
                 "  int (*d)(const void*, const uint64_t*, const uint32_t*, const uint32_t*, const uint8_t*, uint32_t,"
                 " uint32_t, void*, void*, void*, const void*, const void*, void*, void*) = vx_hybrid_device_pieces;\n"
                 "  int64_t (*f)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, const uint8_t*,"
                 " const uint8_t*, size_t, uint8_t*, uint32_t) = vx_hybrid_verify_files;\n"
                 "  int64_t (*r)(vx_ctx*, const char* const*, const uint64_t*, size_t, uint32_t, const uint8_t*,"
                 " const uint8_t*, size_t, size_t, size_t, uint8_t*, uint32_t) = vx_hybrid_verify_files_range;\n"
                 "  (void)d; (void)f; (void)r; return VX_ABI_VERSION != 3; }\n")
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
    assert _lib.lib().vx_hybrid_verify_files.restype is ctypes.c_int64
    assert _lib.lib().vx_hybrid_verify_files_range.restype is ctypes.c_int64


def test_validation_without_gpu(built):
    """Everything the three entries refuse before they touch a device."""
    from vortex_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p

    def einval(rc, word):
        assert rc == _lib.VX_EINVAL, rc
        assert word in L.vx_last_error(), L.vx_last_error()

    good = dict(base=p(0x10000), offs=p(0x20000), lens=p(0x30000), pads=p(0x40000), lw=None, n=4, k=2,
                work=p(0x50000), sha1=p(0x60000), roots=p(0x70000), e1=p(0x80000), e2=p(0x90000), m=p(0xA0000))

    def dev(**kw):
        a = dict(good, **kw)
        return L.vx_hybrid_device_pieces(a["base"], a["offs"], a["lens"], a["pads"], a["lw"], a["n"], a["k"],
                                         a["work"], a["sha1"], a["roots"], a["e1"], a["e2"], a["m"], None)

    for name in ("base", "offs", "lens", "pads", "work"):
        einval(dev(**{name: None}), b"NULL")
    einval(dev(m=None), b"d_matched")
    einval(dev(k=18), b"log2_width > 17")  # piece_length = 16384 << log2_width: above 2 GiB
    einval(dev(n=1 << 30), b"32 bits")
    einval(dev(base=p(0x10008)), b"aligned")
    einval(dev(work=p(0x50008)), b"aligned")
    einval(dev(sha1=p(0x60002)), b"aligned")
    assert dev(n=0) == 0  # n == 0 launches nothing

    paths = (ctypes.c_char_p * 2)(b"/nonexistent/a", b"/nonexistent/b")
    flens = (ctypes.c_uint64 * 2)(100000, 5)
    e1 = ctypes.create_string_buffer(20 * 8)
    e2 = ctypes.create_string_buffer(32 * 8)
    out = ctypes.create_string_buffer(8)

    def files(ctx=None, paths=paths, flens=flens, pl=65536, e1=e1, e2=e2, n=3, out=out):
        return L.vx_hybrid_verify_files(ctx, paths, flens, 2, pl, e1, e2, n, out, 0)

    def frange(first, count, ctx=None, n=3, pl=65536, **kw):
        a = dict(paths=paths, flens=flens, e1=e1, e2=e2, out=out)
        a.update(kw)
        return L.vx_hybrid_verify_files_range(ctx, a["paths"], a["flens"], 2, pl, a["e1"], a["e2"], n, first, count,
                                              a["out"], 0)

    einval(files(), b"NULL context")
    einval(frange(0, 3), b"NULL context")
    # a context that is never dereferenced before the argument checks fail
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, p)
    for name in ("paths", "flens", "e1", "e2", "out"):
        einval(files(ctx, **{name: None}), b"NULL")
        einval(frange(0, 3, ctx, **{name: None}), b"NULL")
    for call in (lambda **kw: files(ctx, **kw), lambda **kw: frange(0, 3, ctx, **kw)):
        einval(call(pl=65536 + 16384), b"power of two")
        einval(call(pl=3 * 16384), b"power of two")
        einval(call(pl=8192), b">= 16384")
        einval(call(pl=0), b">= 16384")
        einval(call(n=2), b"n_pieces")  # 100000 bytes at 64 KiB: 2 pieces, and 5 bytes: 1
        einval(call(n=4), b"n_pieces")
        einval(call(pl=16384, n=3), b"n_pieces")  # 7 + 1 at 16 KiB
    einval(frange(4, 0, ctx), b"range")
    einval(frange(2, 2, ctx), b"range")
    einval(frange(0, 4, ctx), b"range")


# ---- the round planner --------------------------------------------------------

@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("hrd") / "hybrid_rounds_dump"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "hybrid_rounds_dump.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, flens, pl, first, count, stage, chunk=0, budget=0, quiet=0):
    out = subprocess.run([str(exe), str(pl), str(first), str(count), str(stage), str(chunk), str(budget), str(quiet)],
                         input="\n".join(map(str, flens)) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.rstrip("\n").split("\n")
    summary = json.loads(lines[-1])
    rounds = []
    for ln in lines[:-1]:
        tag, *v = ln.split()
        v = [int(x) for x in v]
        if tag == "R":
            rounds.append(dict(new=v[0], end=v[1], w_first=v[2], w_n=v[3], K=v[4], data_blocks=v[5], bytes=v[6],
                               file_bytes=v[7], reads=[], lanes=[], tails=[], table=[]))
        else:
            rounds[-1][{"r": "reads", "l": "lanes", "z": "tails", "t": "table"}[tag]].append(tuple(v))
    return rounds, summary


def _root(rows):
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


def replay(exe, flens, pl, stage, chunk=0, budget=0, first=0, count=-1, seed=1):
    """Run the planner and do what the engine does with its rounds, with
    hashlib in the kernels' place; every property of the issue is asserted on
    the way and the final digests and roots are the model's."""
    from vortex_amd import hybrid

    files = file_bytes(seed, flens)
    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(flens, pl)
    n_all = len(dlen)
    if count < 0:
        count = n_all - first
    rounds, summary = _run(exe, flens, pl, first, count, stage, chunk, budget)
    budget = summary["row_budget"]
    C = summary["chunk"]
    assert C % BLOCK == 0 and 0 < C <= stage
    sha = {}          # piece -> (hashlib object, bytes fed): the chaining state
    done1, done2 = {}, {}
    seen = {}         # (file, byte) coverage: file -> list of (lo, hi) read
    leaves, lw_rows = {}, set()
    window = None
    next_piece = first
    for r in rounds:
        if r["new"]:
            assert window is None, "a window opened before the last one ended"
            window = (r["w_first"], r["w_n"], r["K"])
            assert r["w_first"] == next_piece, "windows tile the range in order"
            assert r["K"] == max(log2w[r["w_first"]:r["w_first"] + r["w_n"]]), "rows at the window's widest log2w"
            assert (r["w_n"] << r["K"]) <= budget, "the row budget holds"
            leaves, lw_rows = {}, set()
        assert window == (r["w_first"], r["w_n"], r["K"])
        w_first, w_n, K = window
        assert r["bytes"] <= stage
        # the reads into the stage
        st = bytearray(r["bytes"])
        filled = []
        for f, off, ln, at, piece in r["reads"]:
            assert at % BLOCK == 0, "stage blocks are 16 KiB aligned"
            assert ln > 0 and off + ln <= flens[f], "no pad byte is ever read"
            assert at + ln <= r["bytes"]
            assert findex[piece] == f and foff[piece] <= off < foff[piece] + dlen[piece]
            st[at:at + ln] = files[f][off:off + ln]
            filled.append((at, at + ln))
            seen.setdefault(f, []).append((off, off + ln))
        filled.sort()
        assert all(a[1] <= b[0] for a, b in zip(filled, filled[1:])), "reads overlap on the stage"
        assert sum(b - a for a, b in filled) == r["file_bytes"]

        def staged(lo, hi):
            return any(a <= lo and hi <= b for a, b in filled)

        # SHA-1 lanes
        for at, ln, pid, poff, tlen in r["lanes"]:
            i = first + pid
            assert at % BLOCK == 0 and ln > 0 and staged(at, at + ln)
            h, fed = sha.setdefault(i, (hashlib.sha1(), 0))
            assert fed == poff, "chunks of a piece are in order"
            assert tlen == dlen[i] + pads[i]
            assert st[at:at + ln] == files[findex[i]][foff[i] + poff:foff[i] + poff + ln]
            h.update(bytes(st[at:at + ln]))
            sha[i] = (h, fed + ln)
            if poff + ln == tlen:  # final: the kernel pads and emits
                assert pads[i] == 0 and i not in done1
                done1[i] = h.digest()
            else:
                assert ln % 64 == 0, "non-final SHA-1 lengths are multiples of 64"
        # tail lanes, after the round's SHA-1 lanes
        for at, dl, pad, pid in r["tails"]:
            i = first + pid
            assert (dl, pad) == (dlen[i], pads[i]) and pad and i not in done1
            h, fed = sha.get(i, (hashlib.sha1(), 0))
            assert fed == dl & ~63, "the tail continues the whole blocks' state"
            rem = dl & 63
            assert at % 4 == 0 and (rem == 0 or staged(at, at + rem))
            assert st[at:at + rem] == files[findex[i]][foff[i] + fed:foff[i] + dl]
            h.update(bytes(st[at:at + rem]) + bytes(pad))
            done1[i] = h.digest()
        # block-table entries
        assert len(r["table"]) >= r["data_blocks"]
        for b, (row, ln) in enumerate(r["table"]):
            assert row < (w_n << K) and row < budget
            assert row not in lw_rows, "leaf rows never collide within a window"
            lw_rows.add(row)
            i = w_first + (row >> K)
            slot = row & ((1 << K) - 1)
            assert slot < (1 << log2w[i])
            if b < r["data_blocks"]:
                want = files[findex[i]][foff[i] + slot * BLOCK:foff[i] + min(dlen[i], (slot + 1) * BLOCK)]
                assert 0 < ln == len(want) and staged(b * BLOCK, b * BLOCK + ln)
                assert st[b * BLOCK:b * BLOCK + ln] == want
                leaves[row] = hashlib.sha256(want).digest()
            else:
                assert ln == 0 and slot * BLOCK >= dlen[i], "an absent slot lies past the piece's data"
                leaves[row] = bytes(32)
        if r["end"]:
            for k in range(w_n):
                i = w_first + k
                rows = [leaves[(k << K) + s] for s in range(1 << log2w[i])]  # KeyError: a row was never written
                done2[i] = _root(rows)
            next_piece = w_first + w_n
            window = None
    assert window is None and next_piece == first + count
    # every data byte of the range in exactly one read, nothing else read
    for f in range(len(flens)):
        mine = sorted(seen.get(f, []))
        want = sorted((foff[i], foff[i] + dlen[i]) for i in range(first, first + count) if findex[i] == f)
        assert all(a[1] <= b[0] for a, b in zip(mine, mine[1:])), "a byte was read twice"
        assert sum(b - a for a, b in mine) == sum(b - a for a, b in want)
        if want:
            assert mine[0][0] == want[0][0] and mine[-1][1] == want[-1][1]
    for i in range(first, first + count):
        data = files[findex[i]][foff[i]:foff[i] + dlen[i]]
        assert done1.get(i) == hybrid.v1_digest(data, pads[i]), f"v1 piece {i}"
        assert done2.get(i) == hybrid.v2_root(data, log2w[i]), f"v2 piece {i}"
    assert set(done1) == set(done2) == set(range(first, first + count))
    return rounds, summary


@pytest.mark.parametrize("name,pl,flens", layouts(), ids=[x[0] for x in layouts()])
def test_planner_layouts(dump_exe, name, pl, flens):
    # the engine's chunk and budget on a 64 MiB stage, then a stage of 8 blocks
    # and a 32 KiB chunk, which cut the same torrent into many windows and rounds
    replay(dump_exe, flens, pl, 64 << 20)
    rounds, s = replay(dump_exe, flens, pl, 8 * BLOCK, chunk=2 * BLOCK)
    assert s["rounds"] > 1 or sum(flens) <= 8 * BLOCK
    if pl == 1 << 20:
        assert s["chunk"] == 2 * BLOCK and any(not r["new"] for r in rounds), "pieces take several chunk rounds"
        # padded pieces end mid-window: a tail lane in a round that is not its window's last
        assert any(r["tails"] and not r["end"] for r in replay(dump_exe, flens, pl, 64 << 20, chunk=4 * BLOCK)[0])
    n = sum(-(-x // pl) for x in flens)
    if n >= 3:
        replay(dump_exe, flens, pl, 8 * BLOCK, chunk=2 * BLOCK, first=1, count=n - 2)


M32 = 32 << 20
LARGE = [  # (piece_length, file_lengths, stage bytes, first, count): trees of 2^11 and 2^12 leaf slots
    (M32, [M32 + 1, 5, 2 * M32 + BLOCK + 7, 3 * BLOCK], 64 << 20, 0, -1),
    (M32, [M32 + 1, 5, 2 * M32 + BLOCK + 7, 3 * BLOCK], 64 << 20, 1, 3),
    (M32, [M32 + 12345, 100, M32 - 1], 8 << 20, 0, -1),   # a stage of a quarter piece
    (64 << 20, [70, (64 << 20) + 65], 64 << 20, 0, -1),   # a stage of exactly one piece
]


@pytest.mark.parametrize("pl,flens,stage,first,count", LARGE, ids=["32MiB", "32MiB-range", "32MiB-stage8", "64MiB"])
def test_planner_large_piece_lengths(dump_exe, pl, flens, stage, first, count):
    """Pieces above 16 MiB: every piece takes many chunk rounds, a padded piece
    of 1 or 5 bytes has a pad of almost the whole piece, and a window holds
    2,048 or 4,096 rows per piece."""
    rounds, s = replay(dump_exe, flens, pl, stage, first=first, count=count)
    assert max(r["K"] for r in rounds) == (pl // BLOCK).bit_length() - 1
    assert any(not r["new"] for r in rounds), "pieces take several chunk rounds"


def test_planner_random_torrents(dump_exe):
    rng = random.Random(20)
    for t in range(20):
        pl = BLOCK << rng.randrange(0, 7)  # 16 KiB .. 1 MiB
        nfiles = rng.randrange(1, 12)
        flens = [rng.choice([0, 1, 63, 64, 65, rng.randrange(1, 3 * pl), rng.randrange(1, BLOCK), pl, pl + 1, 2 * pl])
                 for _ in range(nfiles)]
        if not any(flens):
            flens[0] = 5
        stage = BLOCK * rng.choice([1, 3, 8, 64, 4096])
        chunk = BLOCK * rng.choice([1, 2, 4, 16])
        budget = rng.choice([0, 1 << 17, max(1 << 6, pl // BLOCK)])
        n = sum(-(-x // pl) for x in flens)
        first = rng.randrange(0, n) if t % 3 == 0 else 0
        count = rng.randrange(0, n - first + 1) if t % 3 == 0 else -1
        replay(dump_exe, flens, pl, stage, chunk=chunk, budget=budget, first=first, count=count, seed=100 + t)


def test_planner_row_budget_many_tiny_files(dump_exe):
    """10^5 tiny files at 16 MiB pieces behind one large file: no window takes
    more rows than the budget, and the tiny files do not get 1,024-row trees."""
    pl = 16 << 20
    flens = [3 * pl + 5] + [100] * 100000
    out = subprocess.run([str(dump_exe), str(pl), "0", "-1", str(64 << 20), "0", "0", "1"],
                         input="\n".join(map(str, flens)) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    s = json.loads(out.stdout.strip().splitlines()[-1])
    assert s["pieces"] == 100004 and s["max_window_rows"] <= s["row_budget"] == 1 << 20
    # 4,096 tiny pieces fill a 64 MiB stage at one 16 KiB block each: about 25 windows
    # of one row per piece, not 100,000 trees of 1,024 rows
    assert s["windows"] <= 40 and s["entries"] <= 4 * 1024 + 100000 + 8 * 1024
