"""GPU: hybrid (v1 + v2) torrents — the zero-tail kernel behind
device.hybrid_pieces / vx_hybrid_device_pieces, and the one-pass re-verify from
disk, vx_hybrid_verify_files / _range.

Every expectation is hashlib's: SHA-1 over the data followed by its pad zeros
(hybrid.v1_digest), and the BEP 52 tree over the data alone (hybrid.v2_root).
Everything is bit-exact.  Data is np.random.default_rng(seed) bytes; the device
buffers hold 0xFF wherever no piece has a byte, so a kernel that read past a
piece's data would hash something hashlib did not.
(tests/test_gpu_hybrid_tail_sweep.py runs the tail and finish kernels alone over every tail length.)
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from test_hybrid_cpu import layouts

pytestmark = pytest.mark.gpu

BLOCK = 16384
DATA_LENS = [1, 55, 56, 63, 64, 65, 119, 128, 16383, 16384, 16385]  # ... and piece_length - 1, piece_length


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def edge_shapes(pl):
    """(data_len, pad_len) of the issue's tail-kernel edges at one piece length:
    every data_len padded to the piece length, and unpadded (a last piece)."""
    lens = sorted({d for d in DATA_LENS + [pl - 1, pl] if d <= pl})
    return [(d, pl - d) for d in lens if d < pl] + [(d, 0) for d in lens]


_REF = {}


def reference(pl, shapes, seed):
    """Pieces, widths, digests and roots of a list of shapes, computed once per
    (pl, shapes) and shared; never modified."""
    from vortex_amd import hybrid

    key = (pl, tuple(shapes), seed)
    if key not in _REF:
        full = (pl // BLOCK).bit_length() - 1
        pieces, lw = [], []
        for i, (d, pad) in enumerate(shapes):
            pieces.append(random_bytes(seed * 1000 + i, d))
            own = (-(-d // BLOCK) - 1).bit_length()
            lw.append(own if i % 2 else full)  # a short file's own width, or a long file's last piece
        _REF[key] = (pieces, lw, [hybrid.v1_digest(p, pad) for p, (_, pad) in zip(pieces, shapes)],
                     [hybrid.v2_root(p, w) for p, w in zip(pieces, lw)])
    return _REF[key]


def run_device(gpu, pl, shapes, pieces, lw, exp1=None, exp2=None, damage=None):
    import torch

    from vortex_amd import device as vdev

    offs, at = [], 0
    for p in pieces:
        offs.append(at)
        at += (len(p) + 15) // 16 * 16 + 16
    buf = bytearray(b"\xff" * at)
    for o, p in zip(offs, pieces):
        buf[o:o + len(p)] = p
    if damage is not None:
        buf[offs[damage[0]] + damage[1]] ^= 0x10
    dev = lambda x, dt: torch.tensor(x, dtype=dt, device=gpu)  # noqa: E731
    table = lambda rows: torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(gpu)  # noqa: E731
    sha1, roots, matched = vdev.hybrid_pieces(
        torch.frombuffer(buf, dtype=torch.uint8).to(gpu), dev(offs, torch.int64),
        dev([d for d, _ in shapes], torch.int32), dev([pad for _, pad in shapes], torch.int32),
        (pl // BLOCK).bit_length() - 1, log2w=dev(lw, torch.uint8),
        exp_sha1=table(exp1) if exp1 is not None else None, exp_roots=table(exp2) if exp2 is not None else None)
    torch.cuda.synchronize()
    s, r = sha1.cpu().numpy().tobytes(), roots.cpu().numpy().tobytes()
    n = len(shapes)
    return ([s[20 * i:20 * i + 20] for i in range(n)], [r[32 * i:32 * i + 32] for i in range(n)],
            matched.cpu().tolist() if matched is not None else None)


# ---- the device call ------------------------------------------------------------

@pytest.mark.parametrize("pl", [16384, 65536])
def test_tail_kernel_edges(built, gpu, pl):
    shapes = edge_shapes(pl)
    pieces, lw, want1, want2 = reference(pl, shapes, 1)
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw, want1, want2)
    bad = [(shapes[i], "sha1" if got1[i] != want1[i] else "root") for i in range(len(shapes))
           if got1[i] != want1[i] or got2[i] != want2[i]]
    assert not bad, bad
    assert m == [3] * len(shapes)
    # without expected rows: digests and roots only
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw)
    assert (got1, got2, m) == (want1, want2, None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 255, 256, 257, 600])
def test_mixed_waves(built, gpu, n):
    """The edge shapes of both piece lengths' data lengths at 64 KiB, shuffled,
    so a wave's lanes mix Z from 0 to the maximum and pad-free lanes.  From 257
    pieces on hybrid_prep_kernel and hybrid_merge_kernel (256 lanes a
    workgroup) run a second workgroup, at 600 a third, partial one."""
    pl = 65536
    base = edge_shapes(pl)
    order = np.random.default_rng(n).permutation(len(base)).tolist()
    shapes = [base[order[i % len(base)]] for i in range(n)]
    pieces, lw, want1, want2 = reference(pl, shapes, 2)
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw, want1, want2)
    assert [i for i in range(n) if got1[i] != want1[i]] == []
    assert [i for i in range(n) if got2[i] != want2[i]] == []
    assert m == [3] * n
    # ... and with every third SHA-1 row and every fifth root wrong, so that each lane's verdict is its
    # own: a verdict the merge kernel did not write (its output is not cleared first) cannot pass for one
    e1 = [hashlib.sha1(w).digest() if i % 3 == 0 else w for i, w in enumerate(want1)]
    e2 = [hashlib.sha256(w).digest() if i % 5 == 0 else w for i, w in enumerate(want2)]
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw, e1, e2)
    assert (got1, got2) == (want1, want2)
    assert m == [(0 if i % 3 == 0 else 1) | (0 if i % 5 == 0 else 2) for i in range(n)]


def test_one_byte_of_a_1mib_piece(built, gpu):
    """Z = 16,383 zero blocks behind one mixed block."""
    pl = 1 << 20
    shapes = [(1, pl - 1)]
    pieces, lw, want1, want2 = reference(pl, shapes, 3)
    got1, got2, m = run_device(gpu, pl, shapes, pieces, lw, want1, want2)
    assert (got1, got2, m) == (want1, want2, [3])


def test_each_fault_flips_its_own_bit(built, gpu):
    pl = 16384
    shapes = edge_shapes(pl)
    pieces, lw, want1, want2 = reference(pl, shapes, 1)
    n = len(shapes)
    padded = next(i for i, (d, pad) in enumerate(shapes) if pad and d == 119)
    plain = next(i for i, (d, pad) in enumerate(shapes) if not pad and d == 16383)
    for j in (padded, plain):
        # one wrong byte (the piece's last): both hashes of that piece
        _, _, m = run_device(gpu, pl, shapes, pieces, lw, want1, want2, damage=(j, shapes[j][0] - 1))
        assert m == [0 if i == j else 3 for i in range(n)]
        # one wrong expected row of each kind: that bit only
        e1 = list(want1)
        e1[j] = hashlib.sha1(want1[j]).digest()
        _, _, m = run_device(gpu, pl, shapes, pieces, lw, e1, want2)
        assert m == [2 if i == j else 3 for i in range(n)]
        e2 = list(want2)
        e2[j] = hashlib.sha256(want2[j]).digest()
        _, _, m = run_device(gpu, pl, shapes, pieces, lw, want1, e2)
        assert m == [1 if i == j else 3 for i in range(n)]
    # one table only: the other bit stays clear
    _, _, m = run_device(gpu, pl, shapes, pieces, lw, want1, None)
    assert m == [1] * n
    _, _, m = run_device(gpu, pl, shapes, pieces, lw, None, want2)
    assert m == [2] * n


def test_device_layout_checks(built, gpu):
    import torch

    from vortex_amd import device as vdev

    data = torch.zeros(40000, dtype=torch.uint8, device=gpu)
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=gpu)  # noqa: E731
    with pytest.raises(ValueError, match="neither 0 nor"):
        vdev.hybrid_pieces(data, t([0], torch.int64), t([100], torch.int32), t([5], torch.int32), 0)
    with pytest.raises(ValueError, match="multiple of 16"):
        vdev.hybrid_pieces(data, t([8], torch.int64), t([100], torch.int32), t([0], torch.int32), 0)
    with pytest.raises(ValueError, match="past the data tensor"):
        vdev.hybrid_pieces(data, t([32768], torch.int64), t([16384], torch.int32), t([0], torch.int32), 0)


# ---- the files call ---------------------------------------------------------------

@pytest.fixture(scope="module")
def pool(built, gpu):
    """Three 4 MiB slots of a 64 KiB pool: the 1 MiB pieces take several chunk rounds."""
    from vortex_amd.hash_pool import HashPool

    p = HashPool(65536, slots=3, slot_bytes=4 << 20)
    yield p
    p.close()


def write_files(root, datas, prefix="f"):
    os.makedirs(root, exist_ok=True)
    paths = []
    for k, d in enumerate(datas):
        p = os.path.join(str(root), f"{prefix}{k:04d}.bin")
        with open(p, "wb") as f:
            f.write(d)
        paths.append(p)
    return paths


_TABLES = {}


def tables(name):
    """(pl, flens, file bytes, v1 `pieces` rows, v2 root rows, geometry) of a layout, once."""
    from vortex_amd import hybrid

    if name not in _TABLES:
        _, pl, flens = next(x for x in layouts() if x[0] == name)
        datas = [random_bytes(40 + k, n) for k, n in enumerate(flens)]
        geo = hybrid.hybrid_pieces(flens, pl)
        findex, foff, dlen, pads, log2w = geo
        parts = [datas[f][o:o + d] for f, o, d in zip(findex, foff, dlen)]
        _TABLES[name] = (pl, flens, datas, [hybrid.v1_digest(p, pad) for p, pad in zip(parts, pads)],
                         [hybrid.v2_root(p, w) for p, w in zip(parts, log2w)], geo)
    return _TABLES[name]


def raw_call(pool, paths, flens, pl, e1, e2, first=None, count=None, guard=8):
    """The C call itself: (return value, verdict bytes, the guard bytes behind them)."""
    n = len(e2)
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
    lens = (ctypes.c_uint64 * max(1, len(flens)))(*flens)
    b1 = ctypes.create_string_buffer(b"".join(e1), max(1, 20 * n))
    b2 = ctypes.create_string_buffer(b"".join(e2), max(1, 32 * n))
    cnt = n if count is None else count
    out = ctypes.create_string_buffer(b"\xee" * (cnt + guard), cnt + guard)
    if first is None:
        rc = pool.lib.vx_hybrid_verify_files(pool._h, arr, lens, len(paths), pl, b1, b2, n, out, 0)
    else:
        rc = pool.lib.vx_hybrid_verify_files_range(pool._h, arr, lens, len(paths), pl, b1, b2, n, first, cnt, out, 0)
    return rc, list(out.raw[:cnt]), out.raw[cnt:]


@pytest.mark.parametrize("name", [x[0] for x in layouts()])
def test_files_layouts(pool, tmp_path, name):
    pl, flens, datas, e1, e2, geo = tables(name)
    paths = write_files(tmp_path, datas)
    n = len(e1)
    pool.reset_stats()
    got = pool.verify_hybrid_files(paths, flens, pl, b"".join(e1), b"".join(e2))
    assert got == [(True, True)] * n, [i for i, v in enumerate(got) if v != (True, True)][:10]
    lv, st = pool.last_verify(), pool.stats()
    assert lv["read_bytes"] == sum(flens), "pads are never read, and each byte is read once"
    assert lv["copy_bytes"] <= sum(-(-x // BLOCK) * BLOCK for x in flens)
    assert st["pieces_completed"] == n and st["pieces_mismatched"] == 0 and st["io_errors"] == 0
    assert st["bytes_completed"] == sum(flens)
    if pl == 1 << 20:
        assert lv["chunk_bytes"] == 256 << 10 and lv["rounds"] >= 4  # several chunk rounds per piece
    # a wrong row of each table flips its own bit of its own piece
    for j in sorted({0, n // 2, n - 1}):
        w1 = list(e1)
        w1[j] = hashlib.sha1(e1[j]).digest()
        got = pool.verify_hybrid_files(paths, flens, pl, b"".join(w1), b"".join(e2))
        assert got == [(i != j, True) for i in range(n)]
        w2 = list(e2)
        w2[j] = hashlib.sha256(e2[j]).digest()
        got = pool.verify_hybrid_files(paths, flens, pl, b"".join(e1), b"".join(w2))
        assert got == [(True, i != j) for i in range(n)]


def _flip(path, at):
    with open(path, "r+b") as f:
        f.seek(at)
        b = f.read(1)
        f.seek(at)
        f.write(bytes([b[0] ^ 0x40]))


@pytest.mark.parametrize("name,file,at", [
    ("1MiB", 0, (1 << 20) + 300000),        # a middle chunk of a full piece
    ("1MiB", 0, (5 << 19) + 16),            # the last of the 17 tail bytes of a padded piece
    ("1MiB", 1, 300 * 1024 - 1),            # the last whole block of a padded piece that has no tail bytes
    ("three-files", 0, 0), ("three-files", 2, 65536)])  # one-byte pieces: padded, and the torrent's last
def test_a_damaged_byte_fails_both_bits_of_one_piece(pool, tmp_path, name, file, at):
    pl, flens, datas, e1, e2, geo = tables(name)
    paths = write_files(tmp_path, datas)
    _flip(paths[file], at)
    findex, foff = geo[0], geo[1]
    j = next(i for i in range(len(e1)) if findex[i] == file and foff[i] <= at < foff[i] + pl)
    before = pool.stats()
    rc, got, _ = raw_call(pool, paths, flens, pl, e1, e2)
    assert got == [0 if i == j else 3 for i in range(len(e1))] and rc == 1
    after = pool.stats()
    assert after["pieces_mismatched"] - before["pieces_mismatched"] == 1  # once per piece, not per hash
    assert after["io_errors"] == before["io_errors"]


@pytest.mark.parametrize("case", ["truncated", "missing"])
def test_files_that_lack_bytes_fail_exactly_their_pieces(pool, tmp_path, case):
    pl, flens, datas, e1, e2, geo = tables("1MiB")
    paths = write_files(tmp_path, datas)
    if case == "truncated":
        os.truncate(paths[0], (1 << 20) + 5)  # piece 0 whole, pieces 1 and 2 lack bytes
        fails = [1, 2]
    else:
        os.unlink(paths[1])  # the 300 KiB file: piece 3
        fails = [3]
    before = pool.stats()
    rc, got, _ = raw_call(pool, paths, flens, pl, e1, e2)
    assert got == [0 if i in fails else 3 for i in range(len(e1))]
    after = pool.stats()
    assert rc == len(fails) == after["io_errors"] - before["io_errors"]
    assert after["pieces_mismatched"] == before["pieces_mismatched"]


def test_range_reads_its_span_only(pool, tmp_path):
    pl, flens, datas, e1, e2, geo = tables("200-small")
    paths = write_files(tmp_path, datas)
    dlen = geo[2]
    first, count = 37, 101
    w1 = list(e1)
    w1[first + 5] = bytes(20)
    w1[first - 1] = bytes(20)  # outside the span: not looked at
    rc, got, guard = raw_call(pool, paths, flens, pl, w1, e2, first=first, count=count)
    assert got == [2 if i == 5 else 3 for i in range(count)] and rc == 1
    assert guard == b"\xee" * 8, "entries past the span were written"
    assert pool.last_verify()["read_bytes"] == sum(dlen[first:first + count])
    # the files outside the span may be missing
    ghost = [p if first <= i < first + count else p + ".absent" for i, p in enumerate(paths)]
    rc, got, _ = raw_call(pool, ghost, flens, pl, e1, e2, first=first, count=count)
    assert (rc, got) == (0, [3] * count)
    # a span that cuts a file of several pieces, through the Python call
    pl, flens, datas, e1, e2, geo = tables("1MiB")
    paths = write_files(tmp_path / "m", datas)
    got = pool.verify_hybrid_files(paths, flens, pl, b"".join(e1), b"".join(e2), first=1, count=3)
    assert got == [(True, True)] * 3
    assert pool.last_verify()["read_bytes"] == sum(geo[2][1:4])
    assert pool.verify_hybrid_files(paths, flens, pl, b"".join(e1), b"".join(e2), first=2, count=0) == []


def test_equals_the_two_pass_way_over_materialised_pads(pool, tmp_path):
    """verify_files over files + real zero-filled pad files, then
    verify_merkle_files over the files: the same verdicts, bit for bit."""
    pl, flens, datas, e1, e2, geo = tables("three-files")
    paths = write_files(tmp_path, datas)
    _flip(paths[1], 4321)  # piece 1 is damaged: the verdicts are not all alike
    w2 = list(e2)
    w2[3] = bytes(32)      # ... and the tables disagree about piece 3
    last = max(f for f, n in enumerate(flens) if n)
    all_paths, all_lens = [], []
    for f, (p, n) in enumerate(zip(paths, flens)):
        all_paths.append(p)
        all_lens.append(n)
        if f != last and n % pl:
            pad = os.path.join(str(tmp_path), f"pad{f}")
            with open(pad, "wb") as fh:
                fh.write(bytes(pl - n % pl))
            all_paths.append(pad)
            all_lens.append(pl - n % pl)
    v1, bad1 = pool.verify_files(all_paths, all_lens, pl, b"".join(e1))
    v2, bad2 = pool.verify_merkle_files(paths, flens, pl, b"".join(w2))
    assert bad1 == bad2 == 0 and len(v1) == len(v2) == len(e1)
    got = pool.verify_hybrid_files(paths, flens, pl, b"".join(e1), b"".join(w2))
    assert got == list(zip(v1, v2))
    assert got == [(True, True), (False, False), (True, True), (True, False)]
