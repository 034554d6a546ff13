"""A state-level model of SHA-1, vectorised over lanes.  Host only: numpy, no
torch, no library.

hashlib starts every message at the initial value and keeps its chaining state
to itself, so it cannot say what a kernel that resumes a piece from a given
state, or leaves one behind, should compute.  This model can: a state is a row
of five uint32 words, and every function takes states in and gives states out.
compress() is FIPS 180-4 section 6.1.2 as written there (Ch, Parity, Maj with
plain &, ^, ~, + and rotates), not a restatement of the kernels' forms;
tests/test_sha1_model_cpu.py pins it to hashlib.

  compress(states, words)                  one 64-byte block per lane
  run_blocks(states, buf, offs, lens)      the lens[i] >> 6 whole blocks at buf[offs[i]:]
  pad_blocks(tail, rem, total_len)         the one or two padding blocks of a message
  finish(states, tail, rem, total_len)     ... compressed
  zero_blocks(states, z)                   z[i] all-zero blocks
  digest_rows(states)                      [n, 20] bytes, big-endian words
  tail_rows(buf, offs, rem)                the rem[i] < 64 bytes at buf[offs[i]:], zero-filled to 64
  zero_tail(...)                           a hybrid piece's end: mixed block, zero blocks, final block

Two arguments exist only so that a test can show its shapes tell a subtly wrong
kernel from a right one without running a wrong kernel: `over` (bytes kept
past the tail) and `bits_hi=False` (the bit length cut to 32 bits).
"""
import numpy as np

IV = np.array([0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0], dtype=np.uint32)
_K = [np.uint32(k) for k in (0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xCA62C1D6)]


def iv(n):
    return np.tile(IV, (n, 1))


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def compress(states, words):
    """states [n, 5] uint32, words [n, 16] uint32 (big-endian values of the
    block's bytes) -> the states after the block, [n, 5]."""
    states = np.ascontiguousarray(states, dtype=np.uint32)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    assert states.ndim == 2 and states.shape[1] == 5 and words.shape == (len(states), 16)
    w = [words[:, t] for t in range(16)]
    for t in range(16, 80):
        w.append(_rotl(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    a, b, c, d, e = (states[:, k] for k in range(5))
    for t in range(80):
        if t < 20:
            f = (b & c) ^ (~b & d)
        elif 40 <= t < 60:
            f = (b & c) ^ (b & d) ^ (c & d)
        else:
            f = b ^ c ^ d
        tmp = _rotl(a, 5) + f + e + _K[t // 20] + w[t]
        e, d, c, b, a = d, c, _rotl(b, 30), a, tmp
    return states + np.stack([a, b, c, d, e], axis=1)


def _words(rows):
    """[n, 64] uint8 -> [n, 16] uint32, each word read big-endian."""
    return np.ascontiguousarray(rows, dtype=np.uint8).view(">u4").astype(np.uint32)


def pack(chunks):
    """A list of bytes-like as (buf, offs, lens) for run_blocks / tail_rows."""
    lens = np.array([len(c) for c in chunks], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64) if len(chunks) else lens
    return np.frombuffer(b"".join(bytes(c) for c in chunks) + bytes(64), dtype=np.uint8), offs, lens


def run_blocks(states, buf, offs, lens, live=None):
    """Lane i compresses the lens[i] >> 6 whole 64-byte blocks at buf[offs[i]:];
    a lane that has run out of blocks, or is not live, keeps its state."""
    states = np.array(states, dtype=np.uint32)
    offs = np.asarray(offs, dtype=np.int64)
    nblk = np.asarray(lens, dtype=np.int64) >> 6
    if live is not None:
        nblk = np.where(np.asarray(live, dtype=bool), nblk, 0)
    col = np.arange(64, dtype=np.int64)
    for b in range(int(nblk.max()) if len(nblk) else 0):
        idx = np.flatnonzero(nblk > b)
        states[idx] = compress(states[idx], _words(buf[(offs[idx] + 64 * b)[:, None] + col]))
    return states


def tail_rows(buf, offs, rem, over=0):
    """[n, 64] uint8: the rem[i] bytes at buf[offs[i]:], then zeros.  over[i]
    further bytes of buf are kept after them (a wrong mask; 0 in the model)."""
    offs = np.asarray(offs, dtype=np.int64)
    keep = np.asarray(rem, dtype=np.int64) + over
    col = np.arange(64, dtype=np.int64)
    at = np.minimum(offs[:, None] + col, len(buf) - 1)
    return np.where(col < keep[:, None], buf[at], 0).astype(np.uint8)


def pad_blocks(tail, rem, total_len, bits_hi=True):
    """(first [n, 64], second [n, 64], two [n] bool): the padding of messages of
    total_len[i] bytes whose last rem[i] bytes are tail[i, :rem[i]]: those
    bytes, 0x80, zeros, and the 64-bit big-endian bit length in the last eight
    bytes of the first block (rem <= 55) or of the second.  (rem is given, not
    taken from total_len: the length field is whatever the caller says the
    piece's length is.)  bits_hi=False cuts the bit length to 32 bits."""
    rem = np.asarray(rem, dtype=np.int64)
    n = len(rem)
    total = [int(t) for t in total_len]
    col = np.arange(64, dtype=np.int64)
    first = np.where(col < rem[:, None], np.asarray(tail, dtype=np.uint8).reshape(n, 64), 0).astype(np.uint8)
    first[np.arange(n), rem] = 0x80
    second = np.zeros((n, 64), dtype=np.uint8)
    two = rem > 55
    for i, t in enumerate(total):
        bits = (8 * t) & (2 ** 64 - 1 if bits_hi else 2 ** 32 - 1)
        (second if two[i] else first)[i, 56:] = np.frombuffer(bits.to_bytes(8, "big"), dtype=np.uint8)
    return first, second, two


def finish(states, tail, rem, total_len, bits_hi=True):
    """The states after the one or two padding blocks (pad_blocks)."""
    first, second, two = pad_blocks(tail, rem, total_len, bits_hi)
    states = compress(states, _words(first))
    idx = np.flatnonzero(two)
    states[idx] = compress(states[idx], _words(second[idx]))
    return states


def zero_blocks(states, z):
    """Lane i compresses z[i] all-zero blocks."""
    states = np.array(states, dtype=np.uint32)
    z = np.asarray(z, dtype=np.int64)
    for b in range(int(z.max()) if len(z) else 0):
        idx = np.flatnonzero(z > b)
        states[idx] = compress(states[idx], np.zeros((len(idx), 16), dtype=np.uint32))
    return states


def digest_rows(states):
    return np.ascontiguousarray(np.asarray(states, dtype=np.uint32).astype(">u4")).view(np.uint8).reshape(-1, 20)


def zero_tail(states, buf, tail_offs, lens, pads, over=0, bits_hi=True):
    """The end of a padded hybrid piece, lens[i] data bytes followed by
    pads[i] > 0 zeros, lens[i] + pads[i] a multiple of 64: from states[i] (the
    state after the lens[i] >> 6 whole data blocks; the initial value when
    there is none, states[i] is then ignored) through the block that holds the
    lens[i] & 63 tail bytes at buf[tail_offs[i]:] and zeros, the all-zero
    blocks and the final padding block of the whole length."""
    lens = np.asarray(lens, dtype=np.int64)
    pads = np.asarray(pads, dtype=np.int64)
    assert (pads > 0).all() and ((lens + pads) % 64 == 0).all()
    rem = lens & 63
    s = np.where((lens >> 6 > 0)[:, None], np.asarray(states, dtype=np.uint32), IV)
    idx = np.flatnonzero(rem)
    s[idx] = compress(s[idx], _words(tail_rows(buf, np.asarray(tail_offs, dtype=np.int64)[idx], rem[idx],
                                               np.asarray(over, dtype=np.int64)[idx] if np.ndim(over) else over)))
    s = zero_blocks(s, (pads - np.where(rem, 64 - rem, 0)) >> 6)
    none = np.zeros(len(lens), dtype=np.int64)
    return finish(s, np.zeros((len(lens), 64), dtype=np.uint8), none, lens + pads, bits_hi)
