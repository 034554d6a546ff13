"""GPU: the v2 download path with vx_set_merkle_zero_copy on
(HashPool.merkle_zero_copy): slots whose every piece lies in registered host
memory at a 16-byte aligned address are hashed by merkle_zc_piece_kernel through
the pieces' device mappings; every other v2 slot takes the gathered path and
counts in the trace's fallback_slots.  Completions are checked against the
hashlib model (hybrid.v2_root) and against the same submits with the setting
off; vx_get_stats is the same either way.  No test measures time.
"""
import ctypes
import hashlib
import mmap
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
KiB, MiB = 1024, 1 << 20


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def model_root(data, log2w):
    from vortex_amd import hybrid

    return hybrid.v2_root(data, log2w)


def collect(pool, want, seconds=20.0):
    """Poll (no blocking call, no sleep) until `want` v2 completions have
    arrived; a sticky error is swallowed while results are still due."""
    from vortex_amd._lib import VxError

    out, deadline = [], time.monotonic() + seconds
    while len(out) < want and time.monotonic() < deadline:
        try:
            out.extend(pool.try_iter_merkle())
        except VxError:
            pass
    return out


# forty pieces, 0 B to 2 MiB, own widths 0..7 (mixed in every slot of 16); no slot is all empty
def _forty():
    lens = [0, 1, 15, 16, 17, 255, 256, 257, 511, 513, 4095, 16383, 16384, 16385, 20000, 32768,
            40000, 65535, 65536, 65537, 100000, 131072, 0, 200000, 262144, 262145, 300001, 524288, 600000, 1 * MiB,
            1 * MiB + 3, 1500000, 2 * MiB - 1, 2 * MiB, 7, 49152, 49153, 98304, 163840, 2 * MiB - 16384]
    assert len(lens) == 40
    out = []
    for i, v in enumerate(lens):
        need = max(0, (max(v, 1) - 1) // BLOCK).bit_length()  # the narrowest tree that holds v bytes
        lw = min(7, need + (i % 3 if need + (i % 3) <= 7 else 0))
        assert v <= BLOCK << lw
        out.append((random_bytes(500 + i, v), lw))
    assert {lw for _, lw in out} == set(range(8))
    return out


@pytest.fixture(scope="module")
def forty():
    pieces = _forty()
    roots = [model_root(b, lw) for b, lw in pieces]
    return pieces, roots


class Pool:
    """A registered mmap holding every piece at a 16-byte aligned offset that is no multiple of 256."""

    def __init__(self, pieces):
        offs, cur = [], 0
        for body, _ in pieces:
            cur = (cur + 15) // 16 * 16 + 16
            if cur % 256 == 0:
                cur += 16
            offs.append(cur)
            cur += len(body)
        self.reg = mmap.mmap(-1, cur + 4096)
        self.reg[:] = b"\xA5" * len(self.reg)  # a lane that hashed past a piece's end would get a wrong root
        for o, (body, _) in zip(offs, pieces):
            self.reg[o:o + len(body)] = body
        self.offs = offs

    def view(self, i, n):
        return memoryview(self.reg)[self.offs[i]:self.offs[i] + max(n, 16)]


def submit_forty(pool, host, pieces, roots, plain=()):
    """The forty submits: three slots of 16, 16 and 8 (no flush, so the slot count is exact), then drain."""
    for i, (body, lw) in enumerate(pieces):
        exp = roots[i]
        if i == 11:
            exp = bytes(32)  # a wrong row
        if i == 21:
            exp = None       # no row
        buf = (body if body else bytearray(16)) if i in plain else host.view(i, len(body))
        pool.spawn_merkle(i, 3, buf, len(body), exp, log2w=lw)
    pool.drain()
    got = pool.try_iter_merkle()
    assert pool.pending == 0
    return sorted((r.index, r.hash_matched, r.digest) for r in got)


@pytest.mark.parametrize("placement", ["registered", "plain", "one_plain"])
def test_forty_pieces_three_placements(built, gpu, forty, placement):
    from vortex_amd.hash_pool import HashPool

    pieces, roots = forty
    lens = [len(b) for b, _ in pieces]
    plain = {"registered": (), "plain": tuple(range(40)), "one_plain": (20,)}[placement]
    host = Pool(pieces)
    want = sorted((i, i not in (11, 21), roots[i]) for i in range(40))
    with HashPool(2 * MiB, slots=3, batch_pieces=16, slot_bytes=64 * MiB) as pool:
        pool.register_buffer(host.reg)
        assert pool.merkle_zero_copy is False
        off = submit_forty(pool, host, pieces, roots, plain)
        assert pool.merkle_zero_copy_trace() == {"slots": 0, "pieces": 0, "bytes": 0, "fallback_slots": 0}
        pool.merkle_zero_copy = True
        assert pool.merkle_zero_copy is True
        on = submit_forty(pool, host, pieces, roots, plain)
        trace = pool.merkle_zero_copy_trace()
        st = pool.stats()
        pool.unregister_buffer(host.reg)
    assert on == want and off == want
    zc_slots = {"registered": [range(0, 16), range(16, 32), range(32, 40)], "plain": [],
                "one_plain": [range(0, 16), range(32, 40)]}[placement]
    assert trace == {"slots": len(zc_slots), "pieces": sum(len(r) for r in zc_slots),
                     "bytes": sum(lens[i] for r in zc_slots for i in r), "fallback_slots": 3 - len(zc_slots)}
    assert st["batches"] == 6 and st["pieces_completed"] == 80 and st["bytes_completed"] == 2 * sum(lens)
    assert st["zero_copy_slots"] == 0  # v1's counter: a v2 slot never counts there


def test_wide_piece_takes_the_two_launch_form(built, gpu):
    """A 4 MiB piece is 512 leaves: two tiles of the piece kernel leave their tops for the node kernel."""
    from vortex_amd.hash_pool import HashPool

    pieces = [(random_bytes(31, 4 * MiB), 9), (random_bytes(32, 16384), 0), (random_bytes(33, 4 * MiB - 5), 8),
              (random_bytes(34, 300), 9)]
    host = Pool(pieces)
    with HashPool(8 * MiB, slots=2, batch_pieces=8, slot_bytes=32 * MiB) as pool:
        pool.register_buffer(host.reg)
        pool.merkle_zero_copy = True
        for i, (body, lw) in enumerate(pieces):
            pool.spawn_merkle(i, 0, host.view(i, len(body)), len(body), model_root(body, lw) if i != 1 else bytes(32),
                              log2w=lw)
        pool.drain()
        got = {r.index: r for r in pool.try_iter_merkle()}
        assert pool.stats()["batches"] == 1
        assert pool.merkle_zero_copy_trace() == {"slots": 1, "pieces": 4, "bytes": sum(len(b) for b, _ in pieces),
                                                 "fallback_slots": 0}
        pool.unregister_buffer(host.reg)
    for i, (body, lw) in enumerate(pieces):
        assert got[i].digest == model_root(body, lw) and got[i].hash_matched == (i != 1), i


def test_v1_and_v2_interleaved_on_one_pool(built, gpu):
    """A change of kind launches the open slot; v1 slots count in zero_copy_slots, v2 slots in the trace."""
    from vortex_amd.hash_pool import HashPool

    plen, n = 32 * KiB, 24
    pieces = [(random_bytes(200 + i, plen - (i % 5)), 1) for i in range(n)]
    kinds = [(i // 3) % 2 for i in range(n)]  # v1 x3, v2 x3, ...
    host = Pool(pieces)
    with HashPool(plen, slots=3, batch_pieces=8) as pool:
        pool.register_buffer(host.reg)
        pool.merkle_zero_copy = True
        for i, (b, lw) in enumerate(pieces):
            if kinds[i]:
                pool.spawn_merkle(i, 1, host.view(i, len(b)), len(b), model_root(b, lw))
            else:
                pool.spawn(i, 1, host.view(i, len(b)), len(b), hashlib.sha1(b).digest())
        pool.drain()
        v2, v1 = pool.try_iter_merkle(), pool.try_iter()
        st, trace = pool.stats(), pool.merkle_zero_copy_trace()
        pool.unregister_buffer(host.reg)
    assert sorted(r.index for r in v1) == [i for i in range(n) if not kinds[i]]
    assert sorted(r.index for r in v2) == [i for i in range(n) if kinds[i]]
    assert all(r.hash_matched and r.digest == hashlib.sha1(pieces[r.index][0]).digest() for r in v1)
    assert all(r.hash_matched and r.digest == model_root(pieces[r.index][0], 1) for r in v2)
    assert st["batches"] == 8 and st["zero_copy_slots"] == 4
    assert trace == {"slots": 4, "pieces": 12, "bytes": sum(len(pieces[i][0]) for i in range(n) if kinds[i]),
                     "fallback_slots": 0}


def test_setting_toggled_between_flushes(built, gpu):
    """The setting is read when a slot is launched: on, off and on again while pieces are pending."""
    from vortex_amd.hash_pool import HashPool

    pieces = [(random_bytes(300 + i, 50000 + 1000 * i), 2) for i in range(15)]
    roots = [model_root(b, lw) for b, lw in pieces]
    host = Pool(pieces)
    with HashPool(64 * KiB, slots=3, batch_pieces=64) as pool:
        pool.register_buffer(host.reg)
        for k, on in enumerate((True, False, True)):
            pool.merkle_zero_copy = on
            for i in range(5 * k, 5 * k + 5):
                pool.spawn_merkle(i, 0, host.view(i, len(pieces[i][0])), len(pieces[i][0]), roots[i])
            pool.flush()  # (a slot the flush leaves open is launched by the drain, the setting still on)
            assert pool.pending == 5 * k + 5
        pool.drain()
        got = sorted((r.index, r.hash_matched, r.digest) for r in pool.try_iter_merkle())
        trace = pool.merkle_zero_copy_trace()
        pool.unregister_buffer(host.reg)
    assert got == [(i, True, roots[i]) for i in range(15)]
    assert trace == {"slots": 2, "pieces": 10, "bytes": sum(len(pieces[i][0]) for i in (*range(5), *range(10, 15))),
                     "fallback_slots": 0}


def test_refuse_when_full(built, gpu):
    from vortex_amd._lib import VX_EBUSY, VxError
    from vortex_amd.hash_pool import HashPool

    # Registered 4 MiB pieces: a submit costs the host microseconds and the device 4 MiB over PCIe
    # plus a leaf, so both slots are still in flight when the third submit comes.
    plen = 4 * MiB
    pieces = [(random_bytes(40 + i, plen), 8) for i in range(3)]
    roots = [model_root(b, 8) for b, _ in pieces]
    host = Pool(pieces)
    with HashPool(plen, slots=2, batch_pieces=1, slot_bytes=16 * MiB, refuse_when_full=1) as pool:
        pool.register_buffer(host.reg)
        pool.merkle_zero_copy = True
        accepted, refused = [], None
        for k in range(64):
            i = k % 3
            before = pool.pending
            try:
                pool.spawn_merkle(k, 0, host.view(i, plen), plen, roots[i])
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
        assert pool.merkle_zero_copy_trace() == {"slots": len(accepted), "pieces": len(accepted),
                                                 "bytes": len(accepted) * plen, "fallback_slots": 0}
        pool.unregister_buffer(host.reg)


def test_stats_are_the_same_on_and_off(built, gpu, forty):
    """vx_get_stats field by field for an on run and an off run of the same
    submits, apart from the latency histogram and the times."""
    from vortex_amd.hash_pool import HashPool

    pieces, roots = forty
    host = Pool(pieces)
    runs = {}
    with HashPool(2 * MiB, slots=3, batch_pieces=16, slot_bytes=64 * MiB) as pool:
        pool.register_buffer(host.reg)
        for on in (False, True):
            pool.merkle_zero_copy = on
            pool.reset_stats()
            runs[on] = (submit_forty(pool, host, pieces, roots, plain=(5,)), pool.stats())
        pool.unregister_buffer(host.reg)
    assert runs[True][0] == runs[False][0]
    timed = {"submit_stall_ns", "batch_latency_sum_us", "batch_latency_max_us", "batch_latency_hist"}
    a, b = runs[True][1], runs[False][1]
    assert set(a) == set(b) and set(a) > timed
    assert {k: v for k, v in a.items() if k not in timed} == {k: v for k, v in b.items() if k not in timed}
    assert a["pieces_completed"] == 40 and a["pieces_mismatched"] in (1, 2) and a["batches"] == 3
    assert a["batch_latency_count"] == 3 == sum(a["batch_latency_hist"])


def _live(L):
    out = (ctypes.c_uint64 * 4)()
    L.vx_tuning_live_resources(out)
    return list(out)


def test_device_failure_hands_out_finished_batches_first(built, gpu):
    """The third launch fails (injected on the host, nothing happens on the
    device): the failing submit's piece is not taken, the two launched zero-copy
    batches still come back, then the error; after close the engine holds what
    it held before the pool."""
    from vortex_amd import _lib
    from vortex_amd._lib import VX_EDEVICE, VxError
    from vortex_amd.hash_pool import HashPool

    plen, n = 32 * KiB, 30
    pieces = [(random_bytes(80 + i, plen), 1) for i in range(n)]
    roots = [model_root(b, 1) for b, _ in pieces]
    host = Pool(pieces)
    before = _live(_lib.tuning())
    pool = HashPool(plen, slots=3, batch_pieces=8, hooks=True)
    pool.register_buffer(host.reg)
    pool.merkle_zero_copy = True
    pool.lib.vx_tuning_fail_launch_after(pool._h, 2)
    refused = None
    for i in range(n):
        try:
            pool.spawn_merkle(i, i, host.view(i, plen), plen, roots[i])
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
    assert pool.merkle_zero_copy_trace() == {"slots": 2, "pieces": 16, "bytes": 16 * plen, "fallback_slots": 0}
    pool.close()
    assert _live(_lib.tuning()) == before
