"""GPU: the two hash-proof kernels (merkle_proof_span_kernel,
merkle_proof_walk_kernel) by lane, against hashlib, bit-exact.  The batch of
tests/test_gpu_merkle_layers.py has 60 proofs: one wave of the walk kernel, no
second workgroup, no proof of 64 uncles, no pos with bit 63.  The batches here
(tests/_proof_sweep.py) sit either side of a wave and of a workgroup, spread
named uncle counts over the lanes of a wave, share rows, carry expected rows
that are one bit off, hold bad descriptors among good neighbours, and put a
proof's rows behind the 4 GiB line of d_hashes.

Every batch goes to vx_merkle_device_proofs itself on outputs of n + 1 rows
filled with 0xFF, whose spare row and byte must stay 0xFF; the inputs are
compared with themselves afterwards.  device.merkle_proofs must agree on every
batch it accepts (it refuses the bad descriptors on the host).
"""
import ctypes

import pytest

import _proof_sweep as ps

pytestmark = pytest.mark.gpu


def _dev_rows(blob, dev):
    import torch

    return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev).view(-1, 32)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _raw(gpu, hashes, proofs, expected):
    """vx_merkle_device_proofs on guarded outputs; `hashes` is a device tensor
    the caller compares.  Returns (tops, verdicts)."""
    import torch

    from vortex_amd import _lib

    n = len(proofs)
    arr = _lib.proof_array(proofs)
    raw = bytes(arr)[:24 * n]
    exp = _dev_rows(b"".join(expected), gpu)
    d_proofs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gpu)
    tops = torch.full((n + 1, 32), 0xFF, dtype=torch.uint8, device=gpu)
    matched = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device=gpu)
    rc = _lib.lib().vx_merkle_device_proofs(hashes.data_ptr(), d_proofs.data_ptr(), n, tops.data_ptr(),
                                            exp.data_ptr(), matched.data_ptr(),
                                            int(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == 0, _lib.lib().vx_last_error()
    torch.cuda.synchronize()
    assert _bytes(exp) == b"".join(expected), "the expected rows were written"
    assert _bytes(d_proofs) == raw, "the descriptors were written"
    t, m = _bytes(tops), _bytes(matched)
    assert t[32 * n:] == b"\xFF" * 32, "the spare row of tops was written"
    assert m[n:] == b"\xFF", "the spare verdict was written"
    return [t[32 * k:32 * k + 32] for k in range(n)], list(m[:n])


def _judge(what, proofs, got_tops, got_m, want_tops, want_m):
    bad = [i for i in range(len(proofs)) if got_tops[i] != want_tops[i]]
    assert not bad, (f"{what}: {len(bad)} of {len(proofs)} tops differ from hashlib, first: proof {bad[0]} (wave "
                     f"{bad[0] // 64}, lane {bad[0] % 64}) (pos, row, expected, span, uncles) = {proofs[bad[0]]}; "
                     f"proofs: {bad[:16]}")
    bad = [i for i in range(len(proofs)) if got_m[i] != want_m[i]]
    assert not bad, (f"{what}: {len(bad)} verdicts differ, first: proof {bad[0]} (wave {bad[0] // 64}, lane "
                     f"{bad[0] % 64}) gave {got_m[bad[0]]}, want {want_m[bad[0]]}; proofs: {bad[:16]}")


def _both_entries(gpu, what, b, expected=None, want_m=None):
    """A batch through the raw entry and through device.merkle_proofs."""
    import torch

    from vortex_amd import device as vdev

    expected = b.expected if expected is None else expected
    want_m = b.verdicts() if want_m is None else want_m
    blob = b"".join(b.rows)
    hashes = _dev_rows(blob, gpu)
    tops, m = _raw(gpu, hashes, b.proofs, expected)
    assert _bytes(hashes) == blob, "the hashes were written"
    _judge(what + ", vx_merkle_device_proofs", b.proofs, tops, m, b.tops, want_m)
    d_tops, d_m = vdev.merkle_proofs(hashes, b.proofs, _dev_rows(b"".join(expected), gpu))
    torch.cuda.synchronize()
    t = _bytes(d_tops)
    _judge(what + ", device.merkle_proofs", b.proofs, [t[32 * k:32 * k + 32] for k in range(b.n)], list(_bytes(d_m)),
           b.tops, want_m)
    assert _bytes(hashes) == blob


@pytest.mark.parametrize("n", ps.SIZES)
def test_batch_sizes(built, gpu, n):
    """1 to 600 proofs: spans cycle through 1..512, uncle counts through a mix
    with 0, 1, 63 and 64, pos is 64 random bits; the first proof of 64 uncles
    has bit 63 of pos set."""
    _both_entries(gpu, f"{n} proofs", ps.size_batch(n))


@pytest.mark.parametrize("name", list(ps.WAVE_SHAPES))
def test_wave_shapes(built, gpu, name):
    """130 proofs, so the last wave has two live lanes; the uncle counts over a
    wave's lanes follow the named shape."""
    _both_entries(gpu, name, ps.wave_batch(name))


def test_shared_rows(built, gpu):
    """Proofs that name the same row and overlapping ranges; 40 name expected
    row 0, and the 15 of them whose pos differs do not reach it."""
    b = ps.shared_batch()
    assert b.verdicts().count(0) == 15
    _both_entries(gpu, "shared rows", b)


def test_every_bit_of_the_expected_row_decides(built, gpu):
    """Expected row i is one bit from proof i's top, at bit i of the 256: every
    verdict is 0 and every top still exact; with the true rows every verdict
    is 1.  A compare that dropped a word or masked a bit passes some proof."""
    b = ps.one_bit_batch()
    _both_entries(gpu, "expected rows one bit off", b, ps.wrong_expected(b), [0] * 256)
    _both_entries(gpu, "the true expected rows", b, None, [1] * 256)


@pytest.mark.parametrize("zero_expected", [False, True], ids=["row-0", "zero-row"])
def test_bad_descriptors_among_good_ones(built, gpu, zero_expected):
    """Spans 0, 3, 768, 1024 and uncles 65, 255 at lanes spread over the five
    waves of 300 proofs: verdict 0 and a zero top, which the zero row as the
    expected one does not match; every neighbour is untouched; and the result
    is the same with the rows they name (all in bounds) filled with 0xFF and
    with 0x5A, so those rows go unread."""
    from vortex_amd import device as vdev

    results = []
    for fill in (0xFF, 0x5A):
        b = ps.bad_batch(fill, zero_expected)
        blob = b"".join(b.rows)
        hashes = _dev_rows(blob, gpu)
        tops, m = _raw(gpu, hashes, b.proofs, b.expected)
        assert _bytes(hashes) == blob, "the hashes were written"
        _judge(f"bad descriptors, fill {fill:#x}", b.proofs, tops, m, b.tops, ps.bad_verdicts())
        assert all(tops[i] == bytes(32) and m[i] == 0 for i in ps.BAD_AT)
        results.append((tops, m))
    assert results[0] == results[1]
    first = min(ps.BAD_AT)
    with pytest.raises(ValueError, match=f"proof {first}: span"):
        vdev.merkle_proofs(hashes, b.proofs, _dev_rows(b"".join(b.expected), gpu))


def test_rows_at_and_above_4_gib(built, gpu):
    """d_hashes of 2^27 + 2,048 rows (4 GiB and 64 KiB), allocated and never
    filled: only the rows the four proofs name are written.  The first proof's
    span row lies before the 4 GiB line and its two uncles at and behind it; the
    others start at it and behind it.  A row offset held in 32 bits would read
    row (row - 2^27), which nobody wrote."""
    import torch

    from vortex_amd import device as vdev

    block, proofs, expected, want = ps.far_proofs()
    hashes = torch.empty((ps.FAR_ROWS, 32), dtype=torch.uint8, device=gpu)
    assert hashes.numel() > 1 << 32
    first = ps.FAR_BASE - 1
    written = []
    for _, row, _, span, uncles in proofs:
        lo, hi = row - first, row - first + span + uncles
        hashes[row:row + span + uncles] = _dev_rows(b"".join(block[lo:hi]), gpu)
        written.append((row, lo, hi))
    # what an offset cut to 32 bits would read instead: zero rows, so such a top is wrong for certain
    hashes[:2048] = 0
    tops, m = _raw(gpu, hashes, proofs, expected)
    _judge("rows behind 4 GiB, vx_merkle_device_proofs", proofs, tops, m, want, [1] * 4)
    d_tops, d_m = vdev.merkle_proofs(hashes, proofs, _dev_rows(b"".join(expected), gpu))
    torch.cuda.synchronize()
    assert _bytes(d_tops) == b"".join(want) and _bytes(d_m) == b"\x01" * 4
    for row, lo, hi in written:
        assert _bytes(hashes[row:row + hi - lo]) == b"".join(block[lo:hi]), "the hashes were written"
    assert not bool(hashes[:2048].any())
    del hashes
    torch.cuda.empty_cache()


def test_host_entry_on_600_proofs(built, gpu):
    """HashPool.verify_hash_proofs and vx_merkle_verify_proofs itself (with
    tops_out) on the 600-proof batch, whose verdicts are mixed here: every
    seventh expected row is one bit off."""
    from vortex_amd.hash_pool import HashPool

    b = ps.size_batch(600)
    expected = list(b.expected)
    for i in range(0, 600, 7):
        row = bytearray(expected[i])
        row[i % 32] ^= 0x10
        expected[i] = bytes(row)
    want_m = [0 if i % 7 == 0 else 1 for i in range(600)]
    blob = b"".join(b.rows)
    with HashPool(64 * 1024, slots=2, batch_pieces=8) as pool:
        assert pool.verify_hash_proofs(blob, b.proofs, expected) == [bool(x) for x in want_m]
        assert pool.verify_hash_proofs(blob, b.proofs, b.expected) == [True] * 600
        from vortex_amd._lib import proof_array

        arr = proof_array(b.proofs)
        hbuf = ctypes.create_string_buffer(blob, len(blob))
        ebuf = ctypes.create_string_buffer(b"".join(expected), 32 * 600)
        m_out = ctypes.create_string_buffer(b"\xFF" * 601, 601)
        t_out = ctypes.create_string_buffer(b"\xFF" * (32 * 601), 32 * 601)
        rc = pool.lib.vx_merkle_verify_proofs(pool._h, hbuf, len(b.rows), arr, 600, ebuf, 600, m_out, t_out)
        assert rc == 0, pool.lib.vx_last_error()
        t = t_out.raw
        _judge("vx_merkle_verify_proofs", b.proofs, [t[32 * k:32 * k + 32] for k in range(600)], list(m_out.raw[:600]),
               b.tops, want_m)
        assert m_out.raw[600:] == b"\xFF" and t[32 * 600:] == b"\xFF" * 32
        assert hbuf.raw == blob and bytes(arr)[:24 * 600] == bytes(proof_array(b.proofs))[:24 * 600]
