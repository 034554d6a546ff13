"""The state-level SHA-1 model (tests/_sha1_model.py) against hashlib, and what
the tail sweep's shapes are there for.  Host only.

The model is the yardstick of tests/test_gpu_sha1_chunk_sweep.py and
tests/test_gpu_hybrid_tail_sweep.py wherever a kernel starts from a given
state or leaves one behind, which hashlib cannot follow.  Here it is pinned to
hashlib from the initial value, cut and resumed at every block boundary, and
its 64-bit bit length to struct.pack (a sparse 32 GiB message is out of reach
of hashlib in a test; everything before those eight bytes is pinned by the
short lengths).  The last two tests run the model wrong on purpose, in the two
ways the sweeps' shapes were chosen to notice, and name the lanes that differ.
"""
import hashlib
import struct

import numpy as np

import _sha1_model as md
import _sha1_sweep as sw

LENGTHS = list(range(201)) + [4095, 4096, 4097]


def _model_digests(msgs):
    buf, offs, lens = md.pack(msgs)
    s = md.run_blocks(md.iv(len(msgs)), buf, offs, lens)
    s = md.finish(s, md.tail_rows(buf, offs + (lens & ~63), lens & 63), lens & 63, lens)
    return md.digest_rows(s)


def _hashlib_rows(msgs):
    return np.frombuffer(b"".join(hashlib.sha1(m).digest() for m in msgs), dtype=np.uint8).reshape(len(msgs), 20)


def test_model_from_the_initial_value_equals_hashlib():
    rng = np.random.default_rng(1)
    msgs = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in LENGTHS]
    assert (_model_digests(msgs) == _hashlib_rows(msgs)).all()
    assert md.digest_rows(md.finish(md.iv(1), np.zeros((1, 64), np.uint8), [0], [0])).tobytes() == \
        hashlib.sha1(b"").digest()
    # the round functions one block at a time: "abc" (FIPS 180-4's first example)
    assert _model_digests([b"abc"]).tobytes().hex() == "a9993e364706816aba3e25717850c26c9cd0d89d"


def test_a_piece_cut_at_every_block_boundary_and_resumed():
    """One lane per cut: the blocks before it in one call, the rest from the
    state that call left, and the end as usual."""
    for L in (64 * 9 + 37, 64 * 12, 64 * 7 + 60):
        piece = np.random.default_rng(L).integers(0, 256, L + 64, dtype=np.uint8)
        cuts = np.arange(0, (L >> 6) + 1, dtype=np.int64) * 64
        n = len(cuts)
        zero = np.zeros(n, dtype=np.int64)
        s = md.run_blocks(md.iv(n), piece, zero, cuts)
        assert (s[0] == md.IV).all() and len({r.tobytes() for r in s}) == n
        s = md.run_blocks(s, piece, cuts, L - cuts)
        assert len({r.tobytes() for r in s}) == 1
        tail = md.tail_rows(piece, zero + (L & ~63), zero + (L & 63))
        got = md.digest_rows(md.finish(s, tail, zero + (L & 63), zero + L))
        assert all(r.tobytes() == hashlib.sha1(piece[:L].tobytes()).digest() for r in got)


def test_zero_blocks_and_zero_tail_equal_hashlib():
    rng = np.random.default_rng(3)
    assert md.digest_rows(md.finish(md.zero_blocks(md.iv(3), [0, 1, 5]), np.zeros((3, 64), np.uint8), [0] * 3,
                                    [0, 64, 320])).tobytes() == b"".join(hashlib.sha1(bytes(k)).digest()
                                                                         for k in (0, 64, 320))
    lens = [1, 2, 3, 4, 63, 64, 65, 130, 4095]
    msgs = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
    buf, offs, ln = md.pack(msgs)
    pads = 4096 - ln
    got = md.digest_rows(md.zero_tail(md.run_blocks(md.iv(len(lens)), buf, offs, ln), buf, offs + (ln & ~63), ln, pads))
    assert got.tobytes() == b"".join(hashlib.sha1(m + bytes(4096 - len(m))).digest() for m in msgs)


def test_the_bit_length_is_64_bits_wide():
    totals = [2 ** 29, 2 ** 32 + 64, 2 ** 35, 2 ** 29 + 55, 2 ** 32 + 64 + 56, 2 ** 35 + 63, 2 ** 29 - 1, 4096]
    rem = [t % 64 for t in totals]
    tail = np.full((len(totals), 64), 0x11, dtype=np.uint8)
    first, second, two = md.pad_blocks(tail, rem, totals)
    for i, t in enumerate(totals):
        last = second[i] if rem[i] > 55 else first[i]
        assert two[i] == (rem[i] > 55) and last[56:].tobytes() == struct.pack(">Q", 8 * t)
        assert first[i, :rem[i]].tobytes() == b"\x11" * rem[i] and first[i, rem[i]] == 0x80
        assert not first[i, rem[i] + 1:56 if rem[i] <= 55 else 64].any() and (two[i] or not second[i].any())
        assert not second[i, :56].any()
    # ... and cut to 32 bits it is another block exactly where the length needs more
    f32, s32, _ = md.pad_blocks(tail, rem, totals, bits_hi=False)
    differs = [bool((f32[i] != first[i]).any() or (s32[i] != second[i]).any()) for i in range(len(totals))]
    assert differs == [t >= 2 ** 29 for t in totals]


def test_a_wrong_tail_mask_shows_on_exactly_the_16_bit_lanes():
    """The mixed block keeps rem & 3 bytes of its last word.  A kernel that kept
    three bytes where two belong (a 24-bit mask for the 16-bit one) hashes one
    0xFF that is not the piece's: the model run that way differs from the model
    on every padded lane of the tail grid with rem % 4 == 2, and on no other."""
    g = sw.tail_batch()
    padded = np.flatnonzero(g.pads)
    rem = g.lens[padded] & 63
    right = md.zero_tail(g.states[padded], g.buf, g.tail_offs[padded], g.lens[padded], g.pads[padded])
    wrong = md.zero_tail(g.states[padded], g.buf, g.tail_offs[padded], g.lens[padded], g.pads[padded],
                         over=(rem % 4 == 2).astype(np.int64))
    differs = (right != wrong).any(axis=1)
    assert (differs == (rem % 4 == 2)).all() and differs.sum() >= 900
    # every rem and every count of zero blocks, the lanes without a mixed block among them
    z = (g.pads[padded] - np.where(rem, 64 - rem, 0)) >> 6
    assert set(rem) == set(range(64)) and set(z) == set(range(64)) and ((rem == 0) & (z == 63)).any()
    assert len(g.lens) % 64 and (g.pads == 0).sum() >= 64 + len(padded) // 16


def test_a_32_bit_bit_length_shows_on_exactly_the_long_totals():
    b = sw.chunk_long_batch()
    md_states = md.run_blocks(b.start, b.buf, b.offs, b.lens)
    tail = md.tail_rows(b.buf, b.offs + (b.lens & ~63), b.lens & 63)
    right = md.finish(md_states, tail, b.lens & 63, b.tlens)
    wrong = md.finish(md_states, tail, b.lens & 63, b.tlens, bits_hi=False)
    long_ = np.array([t >= 2 ** 29 for t in b.tlens])
    assert ((right != wrong).any(axis=1) == long_).all() and 0 < long_.sum() < len(long_)
    # every wave of the launch mixes both kinds
    for w in range(0, len(long_), 64):
        assert 0 < long_[w:w + 64].sum() < len(long_[w:w + 64])
    for pl in sw.TAIL_LONG_PIECES + (4096,):
        t = sw.tail_long_batch(pl)
        right = md.zero_tail(t.states, t.buf, t.tail_offs, t.lens, t.pads)
        wrong = md.zero_tail(t.states, t.buf, t.tail_offs, t.lens, t.pads, bits_hi=False)
        assert ((right != wrong).any(axis=1) == (pl >= 2 ** 29)).all()
