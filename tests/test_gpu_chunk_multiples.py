"""GPU: chunk rounds whose block count is a multiple of the block ring.

The chunk kernel (sha1_ragged_split_kernel<true>) runs in two phases switched
at b1 = nfull_min / kBlockRing * kBlockRing.  Chunks are multiples of 4096
bytes, and the other tests use powers of two only: 65536 bytes are 1024 blocks,
1024 % 6 == 4, so phase 2 always has data blocks.  A chunk of 12288 bytes is
192 = 6 * 32 blocks: a wave of non-final chunks then has b1 == nb_wave and
skips phase 2 altogether, in the producer and in the select consumer, and a
final chunk that is a whole chunk has a phase 2 of one padding block.
tests/test_sha1_sweep_cpu.py checks with vx_tuning_chunk_schedule that these
cases really hold such rounds.  Written as test_verify_files_chunk_schedule,
test_strided_batch_chunked and test_gather_batch_chunked (test_gpu_parity.py)
are; verdicts against the oracle, digests against hashlib.
(tests/test_gpu_sha1_chunk_sweep.py runs the chunk kernel alone at every edge of both phases, states compared.)
"""
import hashlib
import mmap
import random

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

RING_CHUNK = 12288             # 192 blocks = kBlockRing * 32
WHOLE = 24 * RING_CHUNK        # 294912: the final chunk is a whole chunk


def _one_bit_off(want, every=7):
    """Expected digests, every 7th one bit (bit i % 8 of byte i % 20) away."""
    exp = list(want)
    for i in range(0, len(want), every):
        d = bytearray(want[i])
        d[i % 20] ^= 1 << (i % 8)
        exp[i] = bytes(d)
    return exp


@pytest.mark.parametrize("pl", [WHOLE, 300000, WHOLE + 56])
@pytest.mark.parametrize("ramp", [0, 1, 5])
@pytest.mark.parametrize("chunk", [RING_CHUNK, 2 * RING_CHUNK])
def test_verify_files_ring_multiple_chunks(built, gpu, tmp_path, chunk, ramp, pl):
    """The multi-file layout of test_verify_files_chunk_schedule: a short last
    piece, one flipped byte, a range call that starts mid-torrent."""
    from vortex_amd.hash_pool import HashPool

    sizes = [3 * pl + 777, 0, 5 * pl + 64, pl // 3]
    paths = []
    for k, L in enumerate(sizes):
        p = tmp_path / f"s{k}.bin"
        p.write_bytes(oracle.gen_piece(17, k, L))
        paths.append(str(p))
    data = b"".join(open(p, "rb").read() for p in paths)
    exp = b"".join(hashlib.sha1(data[i:i + pl]).digest() for i in range(0, len(data), pl))
    n = len(exp) // 20
    with HashPool(pl, slots=3, batch_pieces=4, slot_bytes=4 << 20, verify_chunk=chunk, verify_ramp=ramp) as pool:
        r0 = pool.stats()["chunk_rounds"]
        got, bad = pool.verify_files(paths, sizes, pl, exp, io_threads=3)
        rounds = pool.stats()["chunk_rounds"] - r0
        assert got == [True] * n and bad == 0
        # the chunk path ran: a piece of pl bytes takes at least pl / chunk rounds (the nine pieces fit one
        # window: one wave of eight whole pieces and the short last one, which ends a third of the way in)
        assert n == 9 and rounds >= (pl + chunk - 1) // chunk
        with open(paths[2], "r+b") as f:  # flip a byte in the last chunk of a piece
            f.seek(2 * pl - 100)
            b = f.read(1)
            f.seek(2 * pl - 100)
            f.write(bytes([b[0] ^ 1]))
        got, bad = pool.verify_files(paths, sizes, pl, exp, io_threads=3)
        sub, sub_bad = pool.verify_files(paths, sizes, pl, exp, io_threads=2, first=3, count=n - 4)
    want = oracle.pool_verify_files(paths, sizes, pl, exp, threads=3)
    assert got == want and got.count(False) == 1
    assert sub == want[3:n - 1]


@pytest.mark.parametrize("L,hs_extra,n,last_len", [
    (WHOLE, 0, 70, 100),          # every round of whole rings; the last piece is one short chunk
    (WHOLE + 63, 17, 66, WHOLE),  # a 25th round of 63 bytes (two padding blocks); the last piece ends on a whole chunk
])
def test_strided_batch_ring_multiple_chunks(built, gpu, L, hs_extra, n, last_len):
    from vortex_amd.hash_pool import HashPool

    hs = L + hs_extra
    buf = mmap.mmap(-1, (n - 1) * hs + last_len)
    np.frombuffer(buf, dtype=np.uint8)[:] = np.random.default_rng(L + n).integers(0, 256, len(buf), dtype=np.uint8)
    mv = memoryview(buf)
    pieces = [mv[i * hs:i * hs + (last_len if i == n - 1 else L)] for i in range(n)]
    want = [hashlib.sha1(p).digest() for p in pieces]
    exp = _one_bit_off(want)
    with HashPool(L, slots=3, slot_bytes=4 << 20, batch_chunk=RING_CHUNK) as pool:
        pool.register_buffer(buf)
        r0 = pool.stats()["chunk_rounds"]
        dig = pool.sha1_batch(pieces)
        matched, dig2 = pool.verify_batch(pieces, exp)
        rounds = pool.stats()["chunk_rounds"] - r0
        pool.unregister_buffer(buf)
    assert dig == want and dig2 == want
    assert matched == [i % 7 != 0 for i in range(n)]
    assert rounds >= 2 * ((L + RING_CHUNK - 1) // RING_CHUNK)
    del pieces, mv


def test_gather_batch_ring_multiple_chunks(built, gpu):
    """Pieces in separately registered buffers: the gather form sorts them
    longest first, so the first wave holds the three pieces of WHOLE + 63
    beside pieces of WHOLE: in round 23 some lanes end (one padding block)
    while the others carry on, after 23 rounds without a phase 2."""
    from vortex_amd.hash_pool import HashPool

    lens = [WHOLE] * 70 + [WHOLE + 63] * 3 + [100]
    random.Random(3).shuffle(lens)
    bufs = [mmap.mmap(-1, L + 4096) for L in lens]
    gen = np.random.default_rng(4)
    pieces = []
    for b, L in zip(bufs, lens):
        np.frombuffer(b, dtype=np.uint8)[:] = gen.integers(0, 256, len(b), dtype=np.uint8)  # stale tail bytes too
        pieces.append(memoryview(b)[:L])
    want = [hashlib.sha1(p).digest() for p in pieces]
    exp = _one_bit_off(want)
    with HashPool(max(lens), slots=3, slot_bytes=4 << 20, batch_chunk=RING_CHUNK) as pool:
        for b in bufs:
            pool.register_buffer(b)
        st0 = pool.stats()
        dig = pool.sha1_batch(pieces)
        matched, dig2 = pool.verify_batch(pieces, exp)
        st1 = pool.stats()
        for b in bufs:
            pool.unregister_buffer(b)
    assert dig == want and dig2 == want
    assert matched == [i % 7 != 0 for i in range(len(lens))]
    assert st1["chunk_rounds"] - st0["chunk_rounds"] >= 2 * 25
    # one gather tile per chunk (the chunk is below 64 KiB), for both calls
    assert st1["gather_tiles"] - st0["gather_tiles"] == 2 * sum((L + RING_CHUNK - 1) // RING_CHUNK for L in lens)
    del pieces
