"""GPU: the kernels that finish a hybrid torrent's padded v1 pieces,
sha1_zero_tail_kernel and hybrid_finish_kernel, on their own (through
vx_tuning_zero_tail_kernel and vx_tuning_hybrid_finish_kernel), and
hybrid_prep_kernel with them through the public entries.

Both kernels start from a chaining state, so the yardstick is the state-level
model of tests/_sha1_model.py (pinned to hashlib by
tests/test_sha1_model_cpu.py, which also shows that this grid tells a kernel
with a wrong tail mask or a 32-bit bit length from a right one); the public
entries hash real bytes and are compared with hashlib.  Everything is
bit-exact.  The grid (tests/_sha1_sweep.py, tail_batch): at 4 KiB pieces every
padded length 1..4095, which is every rem = len & 63 (the mixed block keeps
rem & 3 bytes of its last word; rem % 4 == 2 had never run on a GPU) with
every count of zero blocks, shuffled with unpadded lanes, then a wave of
unpadded lanes only.  Rules:

  * the incoming states are random words; a lane without a whole block gets a
    random row too, which it must ignore;
  * every tail sits at a 4-byte aligned offset and is followed by 0xFF bytes
    that are not the piece's; a second run has them inverted;
  * outputs are prefilled with 0xA5 and have a spare row; rows of lanes that
    must not write, and the spare rows, are compared too.
"""
import numpy as np
import pytest

import _sha1_model as md
import _sha1_sweep as sw

pytestmark = pytest.mark.gpu

_cache = {}


def _dev(torch, gpu, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize])).to(gpu)


def _want(b, key):
    """Digest rows of a batch's padded lanes, from the model, once."""
    if key not in _cache:
        p = np.flatnonzero(b.pads)
        _cache[key] = (p, md.digest_rows(md.zero_tail(b.states[p], b.buf, b.tail_offs[p], b.lens[p], b.pads[p])))
    return _cache[key]


def _inverted_after(b):
    buf = b.buf.copy()
    buf[b.after] ^= 0xFF
    assert (buf[~b.after] == b.buf[~b.after]).all() and b.after.sum() > len(b.lens)
    return buf


def _lane_tables(torch, gpu, b, buf):
    n = len(b.lens)
    states = np.concatenate([b.states, np.full((1, 5), 0xA5A5A5A5, dtype=np.uint32)])
    return (_dev(torch, gpu, buf, np.uint8), _dev(torch, gpu, b.tail_offs, np.uint64),
            _dev(torch, gpu, b.lens, np.uint32), _dev(torch, gpu, b.pads, np.uint32),
            _dev(torch, gpu, states, np.uint32), n)


def _zero_tail(torch, gpu, b, piece_length, buf):
    """sha1_zero_tail_kernel over a batch: the digest table [n + 1, 20] (host)."""
    from vortex_amd._lib import check, tuning

    data, offs, lens, pads, states, n = _lane_tables(torch, gpu, b, buf)
    dig = torch.full((n + 1, 20), 0xA5, dtype=torch.uint8, device=gpu)
    check(tuning().vx_tuning_zero_tail_kernel(data.data_ptr(), offs.data_ptr(), lens.data_ptr(), pads.data_ptr(), n,
                                              piece_length, states.data_ptr(), dig.data_ptr(),
                                              int(torch.cuda.current_stream(gpu).cuda_stream)),
          "vx_tuning_zero_tail_kernel", tuning())
    torch.cuda.synchronize()
    return dig.cpu().numpy()


def _check_digests(what, got, b, padded, want, unpadded_rows=None):
    n = len(b.lens)
    bad = padded[(got[padded] != want).any(axis=1)]
    assert bad.size == 0, (f"{what}: {bad.size} digests differ from the model, first: lane {bad[0]} "
                           f"(len {b.lens[bad[0]]}, rem {b.lens[bad[0]] & 63}); rem % 4 of all: "
                           f"{sorted(set((b.lens[bad] & 3).tolist()))}")
    rest = np.flatnonzero(b.pads == 0)
    assert (got[rest] == (0xA5 if unpadded_rows is None else unpadded_rows)).all(), \
        f"{what}: the digest row of an unpadded lane was written"
    assert (got[n] == 0xA5).all(), f"{what}: the spare digest row was written"


# ---------------------------------------------------------------------------
# sha1_zero_tail_kernel
# ---------------------------------------------------------------------------
def test_zero_tail_grid(built, gpu):
    import torch

    b = sw.tail_batch()
    assert len(b.lens) % sw.WAVE
    padded, want = _want(b, "grid")
    runs = []
    for what, buf in (("as laid out", b.buf), ("the bytes after every tail inverted", _inverted_after(b))):
        runs.append(_zero_tail(torch, gpu, b, sw.TAIL_PIECE, buf))
        _check_digests(what, runs[-1], b, padded, want)
    assert (runs[0] == runs[1]).all()


@pytest.mark.parametrize("piece_length", sw.TAIL_LONG_PIECES)
def test_zero_tail_long_totals(built, gpu, piece_length):
    """tail_sched with w[14] != 0: the final block of a 512 MiB and of a 4 GiB
    piece, behind 0 to 3 zero blocks and tails of 0, 2, 58 and 63 bytes."""
    import torch

    b = sw.tail_long_batch(piece_length)
    assert ((b.lens + b.pads) == piece_length).all() and (b.lens >> 6 > 0).all()
    padded, want = _want(b, piece_length)
    _check_digests(f"piece_length {piece_length}", _zero_tail(torch, gpu, b, piece_length, b.buf), b, padded, want)


# ---------------------------------------------------------------------------
# hybrid_finish_kernel
# ---------------------------------------------------------------------------
def _one_bit_off(rows, every):
    """rows with one bit of every `every`-th row flipped, another byte each time."""
    out = rows.copy()
    j = np.arange(0, len(rows), every)
    out[j, (j // every) % rows.shape[1]] ^= (1 << (j % 8)).astype(np.uint8)
    return out


def _finish(torch, gpu, b, dig_in, roots, exp1, exp2, index, flags):
    """hybrid_finish_kernel over a batch: (digest table [n + 1, 20], matched [n + 1]) on the host."""
    from vortex_amd._lib import check, tuning

    data, offs, lens, pads, states, n = _lane_tables(torch, gpu, b, b.buf)
    d_dig = _dev(torch, gpu, dig_in, np.uint8)
    d_matched = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device=gpu)
    t = [_dev(torch, gpu, a, np.uint8) for a in (roots, exp1, exp2, flags)]
    d_index = _dev(torch, gpu, index, np.uint32) if index is not None else None
    check(tuning().vx_tuning_hybrid_finish_kernel(
        data.data_ptr(), offs.data_ptr(), lens.data_ptr(), pads.data_ptr(), n, sw.TAIL_PIECE, states.data_ptr(),
        d_dig.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
        d_index.data_ptr() if index is not None else None, t[3].data_ptr(), d_matched.data_ptr(),
        int(torch.cuda.current_stream(gpu).cuda_stream)), "vx_tuning_hybrid_finish_kernel", tuning())
    torch.cuda.synchronize()
    return d_dig.cpu().numpy(), d_matched.cpu().numpy()


@pytest.mark.parametrize("indexed", [False, True])
def test_hybrid_finish_grid(built, gpu, indexed):
    """The four-way truth table of matched[j] (flags bit x row equal, for each
    hash), padded and unpadded lanes alike; with exp_index the expected rows
    sit in wider tables, in another order."""
    import torch

    b = sw.tail_batch()
    n = len(b.lens)
    padded, want = _want(b, "grid")
    rest = np.flatnonzero(b.pads == 0)
    rng = np.random.default_rng(n + indexed)
    # the digest rows of unpadded lanes are the chunk kernel's: known random rows here
    dig_in = np.full((n + 1, 20), 0xA5, dtype=np.uint8)
    dig_in[rest] = rng.integers(0, 256, (len(rest), 20), dtype=np.uint8)
    sha1_true = dig_in[:n].copy()
    sha1_true[padded] = want
    roots = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rows = n + 9 if indexed else n
    index = rng.permutation(rows)[:n] if indexed else np.arange(n)
    exp1 = rng.integers(0, 256, (rows, 20), dtype=np.uint8)
    exp2 = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
    exp1[index] = _one_bit_off(sha1_true, 7)
    exp2[index] = _one_bit_off(roots, 5)
    j = np.arange(n)
    flags = (j % 4).astype(np.uint8)
    truth = ((flags & 1) & (j % 7 != 0)) | (((flags >> 1) & 1) & (j % 5 != 0)) << 1
    # every verdict on both kinds of lane, and in the wave that has no padded lane
    lone = np.arange(5 * sw.WAVE, 6 * sw.WAVE)
    assert (b.pads[lone] == 0).all() and set(truth[lone]) == {0, 1, 2, 3}
    assert {(int(t), bool(p)) for t, p in zip(truth, b.pads)} == {(t, p) for t in range(4) for p in (False, True)}
    for f in (1, 2, 3):  # a wrong row under a set flag, on both kinds of lane
        wrong = (flags == f) & (truth != f)
        assert (wrong & (b.pads > 0)).any() and (wrong & (b.pads == 0)).any()

    got_dig, m = _finish(torch, gpu, b, dig_in, roots, exp1, exp2, index if indexed else None, flags)
    _check_digests("finish", got_dig, b, padded, want, unpadded_rows=dig_in[rest])
    bad = np.flatnonzero(m[:n] != truth)
    assert bad.size == 0, (f"{bad.size} verdicts wrong, first: lane {bad[0]} (pad {b.pads[bad[0]]}, flags "
                           f"{flags[bad[0]]}) reads {m[bad[0]]}, not {truth[bad[0]]}")
    assert m[n] == 0xA5, "the spare verdict was written"


def test_finish_entry_checks_its_arguments(built, gpu):
    import torch

    from vortex_amd._lib import VX_EINVAL, tuning

    x = torch.zeros(64, dtype=torch.uint8, device=gpu).data_ptr()
    fn = tuning().vx_tuning_hybrid_finish_kernel
    assert fn(x, x, x, x, 1, 4096 + 32, x, x, x, x, x, None, x, x, None) == VX_EINVAL
    assert fn(x, x, x, x, 1, 0, x, x, x, x, x, None, x, x, None) == VX_EINVAL
    assert b"multiple of 64" in tuning().vx_last_error()
    for k in (0, 1, 2, 3, 6, 7, 8, 9, 10, 12, 13):
        args = [x, x, x, x, 1, 4096, x, x, x, x, x, None, x, x, None]
        args[k] = None
        assert fn(*args) == VX_EINVAL and b"NULL" in tuning().vx_last_error()
    assert fn(None, None, None, None, 0, 4096, None, None, None, None, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------
# The public entries: real bytes, hashlib
# ---------------------------------------------------------------------------
PUBLIC_PIECE = 16384
# whole data blocks in front of the tail: the chunk kernel's ring (kBlockRing) at its edges and
# every remainder of it, and the longest piece; the issue's {0, 1, 5, 6, 7, 255} and 2, 4 besides
PUBLIC_BLOCKS = (0, 1, 2, 4, 5, 6, 7, 255)


def _public():
    """(shapes, pieces, v1 digests, v2 roots): every tail length behind each of
    PUBLIC_BLOCKS, all padded, and a few unpadded pieces; hashlib, once."""
    from vortex_amd import hybrid

    if "public" not in _cache:
        shapes = [(64 * f + r, PUBLIC_PIECE - 64 * f - r) for f in PUBLIC_BLOCKS for r in range(64) if 64 * f + r]
        for k, d in enumerate((PUBLIC_PIECE, 1, 64 * 6, 64 * 5 + 2, PUBLIC_PIECE - 2, 64 * 7 + 58)):
            shapes.insert(37 * k + 11, (d, 0))
        rng = np.random.default_rng(len(shapes))
        pieces = [rng.integers(0, 256, d, dtype=np.uint8).tobytes() for d, _ in shapes]
        _cache["public"] = (shapes, pieces, [hybrid.v1_digest(p, pad) for p, (_, pad) in zip(pieces, shapes)],
                            [hybrid.v2_root(p, 0) for p in pieces])
    return _cache["public"]


def test_device_call_every_tail_length(built, gpu):
    """device.hybrid_pieces: hybrid_prep_kernel, the chunk kernel over
    len & ~63 (nfull % kBlockRing of 0, 1, 2, 3, 4 and 5), the tail kernel and
    the merge."""
    import torch

    from vortex_amd import device as vdev

    shapes, pieces, want1, want2 = _public()
    n = len(shapes)
    assert {(d >> 6) % sw.kBlockRing for d, pad in shapes if pad} == set(range(sw.kBlockRing))
    assert {d & 63 for d, pad in shapes if pad} == set(range(64)) and n % sw.WAVE
    offs, size = sw.layout([d for d, _ in shapes], gap=16)
    buf = np.full(size + 64, 0xFF, dtype=np.uint8)
    for o, p in zip(offs, pieces):
        buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    exp1 = _one_bit_off(np.frombuffer(b"".join(want1), dtype=np.uint8).reshape(n, 20), 7)
    exp2 = _one_bit_off(np.frombuffer(b"".join(want2), dtype=np.uint8).reshape(n, 32), 5)
    sha1, roots, matched = vdev.hybrid_pieces(
        torch.from_numpy(buf).to(gpu), torch.tensor(offs, dtype=torch.int64, device=gpu),
        torch.tensor([d for d, _ in shapes], dtype=torch.int32, device=gpu),
        torch.tensor([pad for _, pad in shapes], dtype=torch.int32, device=gpu), 0,
        exp_sha1=torch.from_numpy(exp1).to(gpu), exp_roots=torch.from_numpy(exp2).to(gpu))
    torch.cuda.synchronize()
    got1, got2 = sha1.cpu().numpy(), roots.cpu().numpy()
    bad = [shapes[i] for i in range(n) if got1[i].tobytes() != want1[i]]
    assert not bad, f"{len(bad)} SHA-1 digests differ from hashlib, (len, pad): {bad[:8]}"
    bad = [shapes[i] for i in range(n) if got2[i].tobytes() != want2[i]]
    assert not bad, f"{len(bad)} roots differ from hashlib, (len, pad): {bad[:8]}"
    assert matched.cpu().tolist() == [(i % 7 != 0) | (i % 5 != 0) << 1 for i in range(n)]


def test_download_path_every_mask_and_ring_remainder(built, gpu):
    """64 of those pieces through HashPool.spawn_hybrid / try_iter_hybrid (one
    slot: the chunk kernel over the whole blocks, then hybrid_finish_kernel):
    every rem % 4 behind every nfull % kBlockRing."""
    from vortex_amd.hash_pool import HashPool

    shapes, pieces, want1, want2 = _public()
    tails = (1, 2, 3, 4, 57, 58, 59, 60)
    pick = [i for i, (d, pad) in enumerate(shapes) if pad and (d & 63) in tails]
    assert len(pick) == 64 and {((shapes[i][0] >> 6) % sw.kBlockRing, shapes[i][0] % 4) for i in pick} == \
        {(f, r) for f in range(sw.kBlockRing) for r in range(4)}
    with HashPool(PUBLIC_PIECE, slots=2, batch_pieces=64) as pool:
        for k, i in enumerate(pick):
            pool.spawn_hybrid(i, 3, pieces[i], shapes[i][0], shapes[i][1], want1[i] if k % 7 else bytes(20),
                              want2[i] if k % 5 else bytes(32), log2w=0)
        pool.drain()
        got = {r.index: (r.matched, r.sha1, r.root) for r in pool.try_iter_hybrid()}
    assert got == {i: ((k % 7 != 0) | (k % 5 != 0) << 1, want1[i], want2[i]) for k, i in enumerate(pick)}
