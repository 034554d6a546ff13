"""GPU: the hybrid download path — vx_hybrid_submit / vx_hybrid_submit_piece /
vx_hybrid_poll through HashPool.spawn_hybrid / try_recv_hybrid /
try_iter_hybrid.  One submit gives a piece's SHA-1 over data || implied pad
zeros and its SHA-256 merkle root over the data alone.

Every digest and root is checked against the hashlib models of
vortex_amd/hybrid.py (v1_digest, v2_root).  Placement, slots, ownership,
refusal and failure behave as for vx_submit; v1, v2 and hybrid pieces share one
pool and each kind arrives on its own poll only.  The failures are the injected
host-side ones of the test build; nothing provokes a device fault.
"""
import hashlib
import mmap
import time

import numpy as np
import pytest

from vortex_amd import hybrid

pytestmark = pytest.mark.gpu

KiB, MiB = 1024, 1 << 20
# padded data lengths at 64 KiB pieces: no whole block (1, 55, 56, 63), no mixed
# block (64, 16384), both sides of a block edge and of a leaf edge, one byte short
PADDED = (1, 55, 56, 63, 64, 65, 16383, 16384, 16385, 65535)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def flip(body, at):
    return body[:at] + bytes([body[at] ^ 1]) + body[at + 1:]


def collect(pool, want, seconds=20.0):
    """Poll (no blocking call, no sleep) until `want` hybrid completions have
    arrived; a sticky error is swallowed while results are still due."""
    from vortex_amd._lib import VxError

    out, deadline = [], time.monotonic() + seconds
    while len(out) < want and time.monotonic() < deadline:
        try:
            out.extend(pool.try_iter_hybrid())
        except VxError:
            pass
    return out


def test_forty_pieces_three_placements(built, gpu):
    """40 pieces at 64 KiB (log2w 2), batches of 16, cycling registered-aligned
    (gather), registered at offset 8 (direct copy) and plain bytes (pinned
    stage): ten padded lengths, full pieces, a short unpadded last piece, and
    every kind of planted fault."""
    from vortex_amd.hash_pool import HashPool

    plen, n = 64 * KiB, 40
    lens, pads = [plen] * n, [0] * n
    for k, L in enumerate(PADDED):  # pieces 1, 3, .. 19: every placement sees padded pieces
        lens[2 * k + 1], pads[2 * k + 1] = L, plen - L
    lens[n - 1] = 20000  # the torrent's last piece: short and not padded
    bodies = [random_bytes(300 + i, lens[i]) for i in range(n)]
    sha1 = [hybrid.v1_digest(b, p) for b, p in zip(bodies, pads)]
    roots = [hybrid.v2_root(b, 2) for b in bodies]
    wire = list(bodies)
    wire[11] = flip(bodies[11], 64)      # padded (65 bytes): the byte in the mixed block
    wire[20] = flip(bodies[20], 40000)   # full
    exp1, exp2 = list(sha1), list(roots)
    exp1[13], exp1[22] = bytes(20), flip(sha1[22], 19)  # a wrong SHA-1 row only (padded, full)
    exp2[15], exp2[24] = bytes(32), flip(roots[24], 0)  # a wrong root only (padded, full)
    exp1[17] = exp1[26] = None                          # no SHA-1 row (padded, full)
    exp1[28] = exp2[28] = None                          # nothing to compare with
    want = {i: 3 for i in range(n)}
    want.update({11: 0, 20: 0, 13: 2, 22: 2, 15: 1, 24: 1, 17: 2, 26: 2, 28: 0})
    stride = plen + 4096
    reg = mmap.mmap(-1, n * stride)
    with HashPool(plen, slots=3, batch_pieces=16) as pool:
        pool.register_buffer(reg)
        for i in range(n):
            if i % 3 == 2:
                buf = wire[i] if wire[i] else bytearray(16)
            else:
                off = i * stride + (8 if i % 3 == 1 else 0)
                reg[off:off + lens[i]] = wire[i]
                buf = memoryview(reg)[off:off + plen]
            pool.spawn_hybrid(i, 7, buf, lens[i], pads[i], exp1[i], exp2[i])
            if i % 9 == 8:
                pool.flush()
        assert pool.pending == n
        pool.drain()
        assert pool.try_iter() == [] and pool.try_iter_merkle() == []  # a hybrid piece arrives on its own poll only
        got = pool.try_iter_hybrid()
        assert pool.pending == 0 and pool.try_recv_hybrid() is None
        st = pool.stats()
        pool.unregister_buffer(reg)
    assert sorted(r.index for r in got) == list(range(n))  # every tag exactly once
    for r in got:
        i = r.index
        assert r.conn_id == 7 and r.matched == want[i] and r.hash_matched == (want[i] == 3), (i, r.matched)
        if i in (11, 20):
            assert r.sha1 != sha1[i] and r.root != roots[i]
        else:  # the digest and the root come back whether or not a row was given
            assert r.sha1 == sha1[i] and r.root == roots[i], i
    assert st["pieces_completed"] == n and st["bytes_completed"] == sum(lens)
    assert st["pieces_mismatched"] == 6  # once per piece with a compared side that failed; 17, 26, 28 have none
    assert st["batches"] >= 3 and st["gather_tiles"] >= 14
    assert st["zero_copy_slots"] == 0  # a hybrid slot is always gathered or copied first


def test_short_piece_of_a_short_file(built, gpu):
    """A 20,000-byte single-piece file at 64 KiB pieces: the root over two
    leaves, the digest over 64 KiB."""
    from vortex_amd.hash_pool import HashPool

    body = random_bytes(1, 20000)
    assert hybrid.hybrid_pieces([20000, 5], 65536)[2:] == ([20000, 5], [45536, 0], [1, 0])
    with HashPool(64 * KiB, slots=2, batch_pieces=4) as pool:
        pool.spawn_hybrid(0, 0, body, 20000, 45536, hybrid.v1_digest(body, 45536), hybrid.v2_root(body, 1), log2w=1)
        pool.drain()
        r = pool.try_recv_hybrid()
    assert r.matched == 3 and r.sha1 == hashlib.sha1(body + bytes(45536)).digest() and r.root == hybrid.v2_root(body, 1)


def test_merkle_side_slower_than_the_sha1_side(built, gpu):
    """32 x 16 KiB, one leaf each, unpadded: the SHA-1 chain is 256 blocks, so
    the finish kernel must wait for the merkle stream; a missing join would
    show as a stale root or a clear bit 1."""
    from vortex_amd.hash_pool import HashPool

    bodies = [random_bytes(400 + i, 16 * KiB) for i in range(32)]
    with HashPool(16 * KiB, slots=2, batch_pieces=32) as pool:
        for rep in range(3):  # the slots' root rows are reused: a stale one would be another piece's
            for i, b in enumerate(bodies):
                pool.spawn_hybrid(i, rep, b[rep:] + b[:rep], 16 * KiB, 0, None, hashlib.sha256(b[rep:] + b[:rep]).digest(),
                                  log2w=0)
            pool.drain()
            got = pool.try_iter_hybrid()
            assert sorted(r.index for r in got) == list(range(32))
            for r in got:
                b = bodies[r.index][rep:] + bodies[r.index][:rep]
                assert r.matched == 2 and r.root == hashlib.sha256(b).digest() and r.sha1 == hashlib.sha1(b).digest()


def test_long_tail_and_wide_tree(built, gpu):
    """One 8 MiB piece (512 leaves: the two-launch merkle path) whose data ends
    5 bytes into its second half: about 65,000 zero blocks in the finish kernel."""
    from vortex_amd.hash_pool import HashPool

    L = 4 * MiB + 5
    body = random_bytes(31, L)
    reg = mmap.mmap(-1, 8 * MiB)
    reg[:L] = body
    with HashPool(8 * MiB, slots=2, batch_pieces=8, slot_bytes=32 * MiB) as pool:
        pool.register_buffer(reg)
        pool.spawn_hybrid(0, 0, memoryview(reg), L, 8 * MiB - L, hybrid.v1_digest(body, 8 * MiB - L),
                          hybrid.v2_root(body, 9))
        pool.drain()
        r = pool.try_recv_hybrid()
        pool.unregister_buffer(reg)
    assert r.matched == 3 and r.sha1 == hashlib.sha1(body + bytes(8 * MiB - L)).digest()
    assert r.root == hybrid.v2_root(body, 9)


def test_two_padded_totals_on_one_pool(built, gpu):
    """Padded pieces of 64 KiB and of 32 KiB in all (a short file's single
    piece): a change of the padded total launches the open batch; unpadded
    pieces go with either."""
    from vortex_amd.hash_pool import HashPool

    # (data length, padded total or 0, log2w)
    seq = [(1000, 65536, 2), (65536, 0, 2), (70, 65536, 2), (500, 32768, 1), (20000, 0, 1), (32767, 32768, 1),
           (65535, 65536, 2), (64, 65536, 1)]
    bodies = [random_bytes(500 + i, L) for i, (L, _, _) in enumerate(seq)]
    with HashPool(64 * KiB, slots=3, batch_pieces=64) as pool:
        for i, (L, total, lw) in enumerate(seq):
            pad = total - L if total else 0
            pool.spawn_hybrid(i, 0, bodies[i], L, pad, hybrid.v1_digest(bodies[i], pad), hybrid.v2_root(bodies[i], lw),
                              log2w=lw)
        pool.drain()
        got = {r.index: r for r in pool.try_iter_hybrid()}
        st = pool.stats()
    assert sorted(got) == list(range(len(seq)))
    for i, (L, total, lw) in enumerate(seq):
        pad = total - L if total else 0
        assert got[i].matched == 3 and got[i].sha1 == hybrid.v1_digest(bodies[i], pad), i
        assert got[i].root == hybrid.v2_root(bodies[i], lw), i
    assert st["batches"] == 3  # 64 KiB totals | 32 KiB totals | 64 KiB again


def test_slot_without_and_slot_with_only_padded_pieces(built, gpu):
    from vortex_amd.hash_pool import HashPool

    lens = [65536, 0, 1, 40000, 1, 63, 16385, 65535]
    pads = [0, 0, 0, 0] + [65536 - L for L in lens[4:]]
    bodies = [random_bytes(600 + i, L) for i, L in enumerate(lens)]
    with HashPool(64 * KiB, slots=2, batch_pieces=4) as pool:
        for i, b in enumerate(bodies):
            pool.spawn_hybrid(i, 0, b if b else bytearray(16), lens[i], pads[i], hybrid.v1_digest(b, pads[i]),
                              hybrid.v2_root(b, 2))
        pool.drain()
        got = {r.index: r for r in pool.try_iter_hybrid()}
        assert pool.stats()["batches"] == 2
    for i, b in enumerate(bodies):
        assert got[i].matched == 3 and got[i].sha1 == hybrid.v1_digest(b, pads[i]), i
        assert got[i].root == hybrid.v2_root(b, 2), i
    assert got[1].sha1 == hashlib.sha1(b"").digest()


def test_all_three_kinds_interleaved_on_one_pool(built, gpu):
    """A change of kind launches the open slot; each kind has its own poll."""
    from vortex_amd.hash_pool import HashPool

    plen, n = 32 * KiB, 27
    bodies = [random_bytes(700 + i, plen - (i % 5)) for i in range(n)]
    kinds = [(i // 3) % 3 for i in range(n)]  # v1 x3, v2 x3, hybrid x3, ...
    with HashPool(plen, slots=3, batch_pieces=8) as pool:
        for i, b in enumerate(bodies):
            if kinds[i] == 0:
                pool.spawn(i, 1, b, len(b), hashlib.sha1(b).digest())
            elif kinds[i] == 1:
                pool.spawn_merkle(i, 1, b, len(b), hybrid.v2_root(b, 1))
            else:
                pad = plen - len(b)
                pool.spawn_hybrid(i, 1, b, len(b), pad, hybrid.v1_digest(b, pad), hybrid.v2_root(b, 1))
        assert pool.pending == n
        pool.drain()
        assert pool.pending == n  # results stay queued until polled
        hy = pool.try_iter_hybrid()
        assert pool.pending == n - 9
        v2 = pool.try_iter_merkle()
        v1 = pool.try_iter()
        assert pool.pending == 0
        assert pool.try_iter_hybrid() == [] and pool.try_iter_merkle() == [] and pool.try_iter() == []
        st = pool.stats()
    for got, kind in ((v1, 0), (v2, 1), (hy, 2)):
        assert sorted(r.index for r in got) == [i for i in range(n) if kinds[i] == kind]
    assert all(r.hash_matched and r.digest == hashlib.sha1(bodies[r.index]).digest() for r in v1)
    assert all(r.hash_matched and r.digest == hybrid.v2_root(bodies[r.index], 1) for r in v2)
    for r in hy:
        b = bodies[r.index]
        assert r.matched == 3 and r.sha1 == hybrid.v1_digest(b, plen - len(b)) and r.root == hybrid.v2_root(b, 1)
    assert st["batches"] == 9 and st["pieces_completed"] == n  # one slot per run of three


def test_table_form(built, gpu):
    from vortex_amd._lib import VX_EBUSY, VX_EINVAL, VxError
    from vortex_amd.hash_pool import HashPool

    plen, n = 64 * KiB, 10
    lens = [plen] * n
    lens[4], lens[9] = 33333, 100  # piece 4 ends a file (padded); piece 9 is the torrent's last
    pads = [0] * n
    pads[4] = plen - lens[4]
    bodies = [random_bytes(800 + i, L) for i, L in enumerate(lens)]
    sha1 = [hybrid.v1_digest(b, p) for b, p in zip(bodies, pads)]
    roots = [hybrid.v2_root(b, 2) for b in bodies]
    t1, t2 = list(sha1), list(roots)
    t1[2], t2[4] = bytes(20), bytes(32)  # one row of each table wrong
    with HashPool(plen, slots=2, batch_pieces=4) as pool:
        pool.set_piece_table(b"\x55" * 20 * n)  # the v1 table is another one: it must not be the one compared with
        pool.set_hybrid_tables(b"".join(t1), b"".join(t2))
        for i in reversed(range(n)):  # rows are named, not positional
            pool.spawn_hybrid(i, 0, bodies[i], lens[i], pads[i])
        before = pool.pending
        with pytest.raises(VxError) as e:
            pool.spawn_hybrid(n, 0, bodies[0], plen)  # an index past the table
        assert e.value.code == VX_EINVAL and e.value.refused[0] == n and pool.pending == before == n
        with pytest.raises(VxError) as e:
            pool.set_hybrid_tables(b"".join(sha1), b"".join(roots))  # pieces pending
        assert e.value.code == VX_EBUSY
        # explicit rows beside table rows: not in one slot, both right
        pool.spawn_hybrid(100, 0, bodies[2], lens[2], 0, sha1[2], roots[2])
        pool.drain()
        got = {r.index: r for r in pool.try_iter_hybrid()}
        assert pool.pending == 0
        pool.set_hybrid_tables(b"".join(sha1), b"".join(roots))  # replaces the tables once nothing is pending
        pool.spawn_hybrid(2, 0, bodies[2], lens[2])
        pool.spawn_hybrid(4, 0, bodies[4], lens[4], pads[4])
        pool.drain()
        again = {r.index: r.matched for r in pool.try_iter_hybrid()}
    assert sorted(got) == list(range(n)) + [100]
    for i in range(n):
        assert got[i].matched == {2: 2, 4: 1}.get(i, 3), i
        assert got[i].sha1 == sha1[i] and got[i].root == roots[i], i
    assert got[100].matched == 3
    assert again == {2: 3, 4: 3}


def test_refuse_when_full(built, gpu):
    from vortex_amd._lib import VX_EBUSY, VxError
    from vortex_amd.hash_pool import HashPool

    # Registered 4 MiB pieces: a submit costs the host microseconds and the
    # device a gather over PCIe plus a 65,536-block chain, so both slots are
    # still in flight when the third submit comes.
    plen = 4 * MiB
    reg = mmap.mmap(-1, 3 * plen)
    bodies = [random_bytes(40 + i, plen) for i in range(3)]
    for i, b in enumerate(bodies):
        reg[i * plen:(i + 1) * plen] = b
    sha1 = [hashlib.sha1(b).digest() for b in bodies]
    roots = [hybrid.v2_root(b, 8) for b in bodies]
    with HashPool(plen, slots=2, batch_pieces=1, slot_bytes=16 * MiB, refuse_when_full=1) as pool:
        pool.register_buffer(reg)
        accepted, refused = [], None
        for k in range(64):
            i = k % 3
            before = pool.pending
            try:
                pool.spawn_hybrid(k, 0, memoryview(reg)[i * plen:(i + 1) * plen], plen, 0, sha1[i], roots[i])
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
        assert all(r.matched == 3 and r.sha1 == sha1[r.index % 3] and r.root == roots[r.index % 3] for r in got)
        assert pool.pending == 0 and pool.try_iter_hybrid() == []


def test_failing_submit_does_not_take_the_piece(built, gpu):
    from vortex_amd._lib import VX_ENOMEM, VxError
    from vortex_amd.hash_pool import HashPool

    bodies = [random_bytes(70 + i, 32 * KiB - 7 * i) for i in range(6)]
    pads = [32 * KiB - len(b) for b in bodies]

    def spawn(pool, i):
        pool.spawn_hybrid(i, 0, bodies[i], len(bodies[i]), pads[i], hybrid.v1_digest(bodies[i], pads[i]),
                          hybrid.v2_root(bodies[i], 1))

    with HashPool(32 * KiB, slots=2, batch_pieces=4, hooks=True) as pool:
        pool.lib.vx_tuning_fail_submit_after(pool._h, 3)
        for i in range(3):
            spawn(pool, i)
        with pytest.raises(VxError) as e:
            spawn(pool, 3)
        assert e.value.code == VX_ENOMEM and e.value.refused[0] == 3 and pool.pending == 3
        spawn(pool, 3)  # the context stays usable
        pool.drain()
        got = pool.try_iter_hybrid()
    assert sorted(r.index for r in got) == [0, 1, 2, 3] and all(r.matched == 3 for r in got)


def test_device_failure_hands_out_finished_batches_first(built, gpu):
    """The third launch fails (injected, host side only): the failing submit's
    piece is not taken, the two launched batches still come back from
    vx_hybrid_poll, then the error on every poll; take_unfinished lists
    exactly the rest."""
    from vortex_amd._lib import VX_EDEVICE, VxError
    from vortex_amd.hash_pool import HashPool

    plen, n = 32 * KiB, 30
    bodies = [random_bytes(80 + i, plen - (i % 3)) for i in range(n)]
    pads = [plen - len(b) for b in bodies]
    sha1 = [hybrid.v1_digest(b, p) for b, p in zip(bodies, pads)]
    roots = [hybrid.v2_root(b, 1) for b in bodies]
    pool = HashPool(plen, slots=3, batch_pieces=8, hooks=True)
    pool.lib.vx_tuning_fail_launch_after(pool._h, 2)
    refused = None
    for i in range(n):
        try:
            pool.spawn_hybrid(i, i, bodies[i], len(bodies[i]), pads[i], sha1[i], roots[i])
        except VxError as e:
            assert e.code == VX_EDEVICE
            refused = e.refused
            break
    assert refused is not None and refused[0] == 23  # the third batch fills at the 24th submit
    got = collect(pool, 16)
    assert sorted(r.index for r in got) == list(range(16))
    assert all(r.matched == 3 and r.sha1 == sha1[r.index] and r.root == roots[r.index] for r in got)
    for poll in (pool.try_iter_hybrid, pool.try_iter_merkle, pool.try_iter):  # each poll reports the failure
        with pytest.raises(VxError) as e:
            poll()
        assert e.value.code == VX_EDEVICE
    assert pool.pending == 7
    assert sorted(idx for idx, _, _ in pool.take_unfinished()) == list(range(16, 23))
    pool.close()


def test_equals_the_two_submit_way(built, gpu):
    """The same 12 pieces through spawn (over caller-materialised pads) plus
    spawn_merkle, and through spawn_hybrid: the same digests, roots and verdicts."""
    from vortex_amd.hash_pool import HashPool

    plen = 64 * KiB
    lens = [plen, 1, 63, 64, 4097, 16384, 16385, 40000, 65535, plen, 20000, 777]
    pads = [plen - L for L in lens[:10]] + [0, 0]  # the last two: unpadded short pieces
    bodies = [random_bytes(900 + i, L) for i, L in enumerate(lens)]
    wire = list(bodies)
    wire[4] = flip(bodies[4], 4096)
    exp1 = [hybrid.v1_digest(b, p) for b, p in zip(bodies, pads)]
    exp2 = [hybrid.v2_root(b, 2) for b in bodies]
    exp1[7], exp2[8] = bytes(20), bytes(32)
    with HashPool(plen, slots=3, batch_pieces=16) as pool:
        for i in range(12):
            padded = wire[i] + bytes(pads[i])  # what a caller has to build today
            pool.spawn(i, 0, padded, len(padded), exp1[i])
        for i in range(12):
            pool.spawn_merkle(i, 0, wire[i], lens[i], exp2[i])
        pool.drain()
        v1 = {r.index: r for r in pool.try_iter()}
        v2 = {r.index: r for r in pool.try_iter_merkle()}
        for i in range(12):
            pool.spawn_hybrid(i, 0, wire[i], lens[i], pads[i], exp1[i], exp2[i])
        pool.drain()
        hy = {r.index: r for r in pool.try_iter_hybrid()}
        assert pool.pending == 0
    assert sorted(v1) == sorted(v2) == sorted(hy) == list(range(12))
    for i in range(12):
        assert hy[i].sha1 == v1[i].digest and hy[i].root == v2[i].digest, i
        assert hy[i].matched == int(v1[i].hash_matched) | int(v2[i].hash_matched) << 1, i
    assert [hy[i].matched for i in range(12)] == [3, 3, 3, 3, 0, 3, 3, 2, 1, 3, 3, 3]
