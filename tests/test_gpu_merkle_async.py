"""GPU: the BitTorrent v2 download path — vx_merkle_submit / vx_merkle_poll
through HashPool.spawn_merkle / try_recv_merkle / try_iter_merkle.

Roots are checked against the hashlib model below (16 KiB leaves, the zero
hash beyond the piece, pairwise SHA-256 nodes).  Placement (registered and
aligned -> gather, registered and unaligned -> direct copy, plain -> pinned
stage), slots, ownership, refusal and failure behave as for vx_submit; v1 and
v2 pieces share one pool and each kind arrives on its own poll only.
"""
import hashlib
import mmap
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
KiB, MiB = 1024, 1 << 20


def sha256(b):
    return hashlib.sha256(b).digest()


def model_root(data, log2w):
    rows = [sha256(data[o:o + BLOCK]) if o < len(data) else bytes(32) for o in range(0, BLOCK << log2w, BLOCK)]
    while len(rows) > 1:
        rows = [sha256(rows[k] + rows[k + 1]) for k in range(0, len(rows), 2)]
    return rows[0]


def pad_hash(h):
    out = bytes(32)
    for _ in range(h):
        out = sha256(out + out)
    return out


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def collect(pool, want, v1=False, seconds=20.0):
    """Poll (no blocking call, no sleep) until `want` completions of one kind
    have arrived; a sticky error is swallowed while results are still due."""
    from vortex_amd._lib import VxError

    out, deadline = [], time.monotonic() + seconds
    while len(out) < want and time.monotonic() < deadline:
        try:
            out.extend(pool.try_iter() if v1 else pool.try_iter_merkle())
        except VxError:
            pass
    return out


def test_forty_pieces_three_placements(built, gpu):
    """40 x 64 KiB, batches of 16, cycling registered-aligned (gather),
    registered at offset 8 (direct copy) and plain bytes (pinned stage)."""
    from vortex_amd.hash_pool import HashPool

    plen, n = 64 * KiB, 40
    stride = plen + 4096
    reg = mmap.mmap(-1, n * stride)
    bodies = [random_bytes(100 + i, plen) for i in range(n)]
    roots = [model_root(b, 2) for b in bodies]
    with HashPool(plen, slots=3, batch_pieces=16) as pool:
        pool.register_buffer(reg)
        for i, body in enumerate(bodies):
            exp = roots[i]
            if i == 11:
                body = body[:40000] + bytes([body[40000] ^ 1]) + body[40001:]  # corrupted on the wire
            if i == 20:
                exp = None
            if i % 3 == 2:
                buf = body
            else:
                off = i * stride + (8 if i % 3 == 1 else 0)
                reg[off:off + plen] = body
                buf = memoryview(reg)[off:off + plen]
            pool.spawn_merkle(i, 7, buf, plen, exp)
            if i % 9 == 8:
                pool.flush()
        assert pool.pending == n
        pool.drain()
        assert pool.try_iter() == []  # a v2 piece never arrives on the v1 poll
        got = pool.try_iter_merkle()
        assert pool.pending == 0 and pool.try_recv_merkle() is None
        st = pool.stats()
        pool.unregister_buffer(reg)
    assert sorted(r.index for r in got) == list(range(n))  # every tag exactly once
    for r in got:
        assert r.conn_id == 7 and len(r.digest) == 32
        if r.index == 11:
            assert not r.hash_matched and r.digest != roots[11]
        elif r.index == 20:
            assert r.digest == roots[20] and not r.hash_matched  # no expected root: the root comes back, matched 0
        else:
            assert r.hash_matched and r.digest == roots[r.index], r.index
    assert st["pieces_completed"] == n and st["bytes_completed"] == n * plen
    assert st["batches"] >= 3 and st["gather_tiles"] >= 14
    assert st["zero_copy_slots"] == 0  # a v2 slot is always gathered or copied first
    # piece 11 is corrupt (piece 20, with no root to match in a batch that compares, may count as well)
    assert st["pieces_mismatched"] in (1, 2)


def test_short_empty_and_mixed_widths_in_one_slot(built, gpu):
    from vortex_amd.hash_pool import HashPool

    cases = [(random_bytes(1, 20000), 2), (b"", 2), (b"", 0), (random_bytes(2, 16384), 0), (random_bytes(3, 65536), 2),
             (random_bytes(4, 1), 0), (random_bytes(5, 16385), 2), (random_bytes(6, 49153), 2)]
    with HashPool(64 * KiB, slots=2, batch_pieces=64) as pool:
        for i, (body, lw) in enumerate(cases):
            pool.spawn_merkle(i, 0, body if body else bytearray(16), len(body), model_root(body, lw), log2w=lw)
        pool.drain()
        got = {r.index: r for r in pool.try_iter_merkle()}
        assert pool.stats()["batches"] == 1
    assert sorted(got) == list(range(len(cases)))
    for i, (body, lw) in enumerate(cases):
        assert got[i].hash_matched and got[i].digest == model_root(body, lw), i
    assert got[1].digest == pad_hash(2) and got[2].digest == pad_hash(0) == bytes(32)


def test_default_width_is_piece_length_over_block(built, gpu):
    from vortex_amd.hash_pool import HashPool

    body = random_bytes(9, 128 * KiB - 3)
    with HashPool(128 * KiB, slots=2, batch_pieces=4) as pool:
        pool.spawn_merkle(0, 0, body, len(body), model_root(body, 3))
        pool.drain()
        r = pool.try_recv_merkle()
    assert r.hash_matched and r.digest == model_root(body, 3)


def test_v1_and_v2_interleaved_on_one_pool(built, gpu):
    """A change of kind launches the open slot; each kind has its own poll."""
    from vortex_amd.hash_pool import HashPool

    plen, n = 32 * KiB, 24
    bodies = [random_bytes(200 + i, plen - (i % 5)) for i in range(n)]
    kinds = [(i // 3) % 2 for i in range(n)]  # v1 x3, v2 x3, ...
    with HashPool(plen, slots=3, batch_pieces=8) as pool:
        for i, b in enumerate(bodies):
            if kinds[i]:
                pool.spawn_merkle(i, 1, b, len(b), model_root(b, 1))
            else:
                pool.spawn(i, 1, b, len(b), hashlib.sha1(b).digest())
        assert pool.pending == n
        pool.drain()
        assert pool.pending == n  # results stay queued until polled
        v2 = pool.try_iter_merkle()
        assert pool.pending == n - len(v2) == 12
        v1 = pool.try_iter()
        assert pool.pending == 0
        assert pool.try_iter_merkle() == [] and pool.try_iter() == []
        st = pool.stats()
    assert sorted(r.index for r in v1) == [i for i in range(n) if not kinds[i]]
    assert sorted(r.index for r in v2) == [i for i in range(n) if kinds[i]]
    for r in v1:
        assert r.hash_matched and r.digest == hashlib.sha1(bodies[r.index]).digest()
    for r in v2:
        assert r.hash_matched and r.digest == model_root(bodies[r.index], 1)
    assert st["batches"] == 8 and st["pieces_completed"] == n  # one slot per run of three


def test_wide_piece_takes_the_two_launch_path(built, gpu):
    """max_piece_len 8 MiB: one 8 MiB piece (512 leaves) beside a 16 KiB one."""
    from vortex_amd.hash_pool import HashPool

    big, small = random_bytes(31, 8 * MiB), random_bytes(32, 16384)
    reg = mmap.mmap(-1, 8 * MiB)
    reg[:] = big
    with HashPool(8 * MiB, slots=2, batch_pieces=8, slot_bytes=32 * MiB) as pool:
        pool.register_buffer(reg)
        pool.spawn_merkle(0, 0, memoryview(reg), 8 * MiB, model_root(big, 9))
        pool.spawn_merkle(1, 0, small, 16384, model_root(small, 0), log2w=0)
        pool.spawn_merkle(2, 0, small, 16384, bytes(32), log2w=0)
        pool.drain()
        got = {r.index: r for r in pool.try_iter_merkle()}
        assert pool.stats()["batches"] == 1
        pool.unregister_buffer(reg)
    assert got[0].hash_matched and got[0].digest == model_root(big, 9)
    assert got[1].hash_matched and got[1].digest == model_root(small, 0) == sha256(small)
    assert not got[2].hash_matched and got[2].digest == sha256(small)


def test_refuse_when_full(built, gpu):
    from vortex_amd._lib import VX_EBUSY, VxError
    from vortex_amd.hash_pool import HashPool

    # Registered 4 MiB pieces: a submit costs the host microseconds and the
    # device a gather over PCIe plus a leaf, so both slots are still in flight
    # when the third submit comes.
    plen = 4 * MiB
    reg = mmap.mmap(-1, 3 * plen)
    bodies = [random_bytes(40 + i, plen) for i in range(3)]
    for i, b in enumerate(bodies):
        reg[i * plen:(i + 1) * plen] = b
    roots = [model_root(b, 8) for b in bodies]
    with HashPool(plen, slots=2, batch_pieces=1, slot_bytes=16 * MiB, refuse_when_full=1) as pool:
        pool.register_buffer(reg)
        accepted, refused = [], None
        for k in range(64):
            i = k % 3
            before = pool.pending
            try:
                pool.spawn_merkle(k, 0, memoryview(reg)[i * plen:(i + 1) * plen], plen, roots[i])
                accepted.append(k)
            except VxError as e:
                assert e.code == VX_EBUSY and e.refused[0] == k
                assert pool.pending == before  # a refusal changes nobody's owner
                refused = k
                break
        assert refused is not None and len(accepted) >= 2
        assert pool.stats()["submits_refused"] == 1
        got = collect(pool, len(accepted))
        assert sorted(r.index for r in got) == accepted  # every accepted tag, never the refused one
        assert all(r.hash_matched and r.digest == roots[r.index % 3] for r in got)
        assert pool.pending == 0 and pool.try_iter_merkle() == []


def test_bulk_calls_are_busy_while_a_v2_piece_is_pending(built, gpu):
    from vortex_amd._lib import VX_EBUSY, VxError
    from vortex_amd.hash_pool import HashPool

    body = random_bytes(50, 64 * KiB)
    root = model_root(body, 2)
    with HashPool(64 * KiB, slots=2, batch_pieces=8) as pool:
        pool.spawn_merkle(0, 0, body, len(body), root)
        for call in (lambda: pool.verify_merkle([body], [root], 64 * KiB),
                     lambda: pool.verify_batch([body], [hashlib.sha1(body).digest()])):
            with pytest.raises(VxError) as e:
                call()
            assert e.value.code == VX_EBUSY
        pool.drain()
        with pytest.raises(VxError) as e:  # finished but not yet polled: still the caller's to collect
            pool.verify_merkle([body], [root], 64 * KiB)
        assert e.value.code == VX_EBUSY
        r = pool.try_recv_merkle()
        assert r.hash_matched and r.digest == root and pool.pending == 0
        assert pool.verify_merkle([body], [root], 64 * KiB) == ([True], [root])


def test_bad_arguments_take_nothing(built, gpu):
    from vortex_amd._lib import VX_EINVAL, VX_ERANGE, VxError
    from vortex_amd.hash_pool import HashPool

    buf = bytearray(256 * KiB)
    with HashPool(64 * KiB, slots=2, batch_pieces=8) as pool:
        pool.spawn_merkle(0, 0, buf, 16384, None, log2w=0)
        for args, code in (((buf, 16385, None, 0), VX_EINVAL),       # longer than its tree
                           ((buf, 65536, None, 1), VX_EINVAL),
                           ((buf, 16384, None, 3), VX_EINVAL),       # a tree wider than max_piece_len
                           ((buf, 16384, None, 18), VX_EINVAL),
                           ((buf, 65537, None, 2), VX_ERANGE),       # longer than max_piece_len
                           ((buf, 256 * KiB, None, 4), VX_ERANGE)):
            with pytest.raises(VxError) as e:
                pool.spawn_merkle(1, 0, args[0], args[1], args[2], log2w=args[3])
            assert e.value.code == code and e.value.refused[0] == 1
            assert pool.pending == 1
        with pytest.raises(ValueError):
            pool.spawn_merkle(1, 0, buf, 16384, b"short", log2w=0)
        pool.drain()
        r = pool.try_iter_merkle()
        assert len(r) == 1 and r[0].digest == sha256(bytes(16384)) and pool.pending == 0
    # a max_piece_len that is no power of two rounds up: 40000 bytes fit a tree of 4 leaves
    body = random_bytes(60, 40000)
    with HashPool(40000, slots=2, batch_pieces=8) as pool:
        pool.spawn_merkle(0, 0, body, 40000, model_root(body, 2), log2w=2)
        pool.drain()
        assert pool.try_recv_merkle().hash_matched


def test_failing_submit_does_not_take_the_piece(built, gpu):
    from vortex_amd._lib import VX_ENOMEM, VxError
    from vortex_amd.hash_pool import HashPool

    bodies = [random_bytes(70 + i, 32 * KiB) for i in range(6)]
    with HashPool(32 * KiB, slots=2, batch_pieces=4, hooks=True) as pool:
        pool.lib.vx_tuning_fail_submit_after(pool._h, 3)
        for i in range(3):
            pool.spawn_merkle(i, 0, bodies[i], 32 * KiB, model_root(bodies[i], 1))
        with pytest.raises(VxError) as e:
            pool.spawn_merkle(3, 0, bodies[3], 32 * KiB, model_root(bodies[3], 1))
        assert e.value.code == VX_ENOMEM and e.value.refused[0] == 3 and pool.pending == 3
        pool.spawn_merkle(3, 0, bodies[3], 32 * KiB, model_root(bodies[3], 1))  # the context stays usable
        pool.drain()
        got = pool.try_iter_merkle()
    assert sorted(r.index for r in got) == [0, 1, 2, 3] and all(r.hash_matched for r in got)


def test_device_failure_hands_out_finished_batches_first(built, gpu):
    """The third launch fails (injected, host side only): the failing submit's
    piece is not taken, the two launched batches still come back from
    vx_merkle_poll, then the error; pending is the tags never returned."""
    from vortex_amd._lib import VX_EDEVICE, VxError
    from vortex_amd.hash_pool import HashPool

    plen, n = 32 * KiB, 30
    bodies = [random_bytes(80 + i, plen) for i in range(n)]
    roots = [model_root(b, 1) for b in bodies]
    pool = HashPool(plen, slots=3, batch_pieces=8, hooks=True)
    pool.lib.vx_tuning_fail_launch_after(pool._h, 2)
    refused = None
    for i in range(n):
        try:
            pool.spawn_merkle(i, i, bodies[i], plen, roots[i])
        except VxError as e:
            assert e.code == VX_EDEVICE
            refused = e.refused
            break
    assert refused is not None and refused[0] == 23  # the third batch fills at the 24th submit
    got = collect(pool, 16)
    assert sorted(r.index for r in got) == list(range(16))
    assert all(r.hash_matched and r.digest == roots[r.index] for r in got)
    for poll in (pool.try_iter_merkle, pool.try_iter):  # each poll reports the failure once its queue is empty
        with pytest.raises(VxError) as e:
            poll()
        assert e.value.code == VX_EDEVICE
    assert pool.pending == 7
    assert sorted(idx for idx, _, _ in pool.take_unfinished()) == list(range(16, 23))
    pool.close()


def test_stats_count_v2_pieces(built, gpu):
    from vortex_amd.hash_pool import HashPool

    lens = [65536, 40000, 0, 16384, 1, 65535]
    bodies = [random_bytes(90 + i, ln) for i, ln in enumerate(lens)]
    with HashPool(64 * KiB, slots=2, batch_pieces=4) as pool:
        pool.reset_stats()
        for i, b in enumerate(bodies):
            exp = model_root(b, 2) if i != 4 else bytes(32)
            pool.spawn_merkle(i, 0, b if b else bytearray(16), len(b), exp)
        pool.drain()
        got = pool.try_iter_merkle()
        st = pool.stats()
    assert [r.hash_matched for r in sorted(got, key=lambda r: r.index)] == [True, True, True, True, False, True]
    assert (st["pieces_completed"], st["bytes_completed"], st["pieces_mismatched"], st["batches"]) == \
        (6, sum(lens), 1, 2)
    assert st["batch_latency_count"] == 2 and sum(st["batch_latency_hist"]) == 2
