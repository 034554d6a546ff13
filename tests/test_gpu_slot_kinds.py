"""GPU: what a slot keeps per piece kind (vx_slots.hip: fits, record_rows,
harvest, uncommit) where the other download-path tests are thin: a v1 slot
changing between explicit rows and table rows, slots whose pieces only partly
carry an expected row (v1 and v2), and a hybrid piece leaving its slot again
when the launch it triggers fails.

Pieces are at most 64 KiB, from registered (gathered) and plain (staged)
sources; digests and roots are checked against hashlib and
vortex_amd.hybrid.v2_root.  The failure is the injected host-side one of the
test build; nothing provokes a device fault.
"""
import hashlib
import mmap

import numpy as np
import pytest

from vortex_amd import hybrid

pytestmark = pytest.mark.gpu

KiB = 1024
PLEN = 64 * KiB
STRIDE = PLEN + 4096
# both sides of a SHA-1 block edge and of a 16 KiB leaf edge, empty and full pieces
LENS = (0, 1, 63, 64, 65, 16385, PLEN, 40000, 16384)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def source(reg, i, body):
    """Even pieces from the registered mmap (16-byte aligned: gathered), odd
    ones as plain bytes (the pinned stage)."""
    if i % 2:
        return body if body else bytearray(16)
    reg[i * STRIDE:i * STRIDE + len(body)] = body
    return memoryview(reg)[i * STRIDE:i * STRIDE + PLEN]


def spawn_without_row(pool, index, buf, n):
    """vx_submit with expected = NULL: HashPool.spawn reads None as 'the table'."""
    from vortex_amd._lib import check
    from vortex_amd.hash_pool import _addr_of

    addr, keep = _addr_of(buf)
    tag = pool._next_tag
    pool._next_tag += 1
    check(pool.lib.vx_submit(pool._h, tag, addr, n, None), "vx_submit", pool.lib)
    pool._inflight[tag] = (index, 0, buf, keep)


def test_v1_slot_changes_form(built, gpu):
    """Three explicit-row pieces, three table pieces, three explicit again on
    one pool: a change of form launches the open slot, so three batches; one
    table row and one explicit row are wrong."""
    from vortex_amd.hash_pool import HashPool

    bodies = [random_bytes(10 + i, L) for i, L in enumerate(LENS)]
    sha1 = [hashlib.sha1(b).digest() for b in bodies]
    table = list(sha1)
    table[4] = bytes(20)
    reg = mmap.mmap(-1, len(LENS) * STRIDE)
    with HashPool(PLEN, slots=3, batch_pieces=8) as pool:
        pool.register_buffer(reg)
        pool.set_piece_table(b"".join(table))
        for i, b in enumerate(bodies):
            by_table = 3 <= i < 6
            exp = None if by_table else (sha1[i] if i != 7 else sha1[0])
            pool.spawn(i, 2, source(reg, i, b), len(b), exp)
        pool.drain()
        got = {r.index: r for r in pool.try_iter()}
        st = pool.stats()
        pool.unregister_buffer(reg)
    assert sorted(got) == list(range(len(LENS)))
    for i in range(len(LENS)):
        assert got[i].digest == sha1[i], i
        assert got[i].hash_matched == (i not in (4, 7)), i
    assert st["batches"] == 3 and st["pieces_completed"] == len(LENS) and st["pieces_mismatched"] == 2


def mixed_rows(pool, reg, spawn, rowless, digest):
    """Slot A (8 pieces = batch_pieces): 0-2 without a row, 3, 4 right, 5 wrong,
    6 without a row, 7 right.  Slot B: 3 pieces, none with a row."""
    lens = list(LENS[:8]) + [65, 16385, 1]
    bodies = [random_bytes(40 + i, L) for i, L in enumerate(lens)]
    want = [digest(b) for b in bodies]
    for i, b in enumerate(bodies):
        if i in (3, 4, 7):
            spawn(i, source(reg, i, b), len(b), want[i])
        elif i == 5:
            spawn(i, source(reg, i, b), len(b), want[0])
        else:
            rowless(i, source(reg, i, b), len(b))
    pool.drain()
    return want


def check_mixed(got, want, st):
    assert sorted(got) == list(range(11))
    for i in range(11):
        assert got[i].digest == want[i], i
        assert got[i].hash_matched == (i in (3, 4, 7)), i
    assert st["batches"] == 2 and st["pieces_completed"] == 11
    assert st["pieces_mismatched"] == 5


def test_v1_slot_with_some_expected_rows(built, gpu):
    """A slot whose first pieces carry no expected row and whose later ones do.
    Every digest is right; a piece without a row reports matched == 0.

    pieces_mismatched is 5: harvest counts every piece of a slot that has any
    expected row and did not match, so slot A's four pieces without a row (they
    are compared with a zero row) count beside the planted one; slot B has no
    row at all and counts nothing."""
    from vortex_amd.hash_pool import HashPool

    reg = mmap.mmap(-1, 11 * STRIDE)
    with HashPool(PLEN, slots=2, batch_pieces=8) as pool:
        pool.register_buffer(reg)
        want = mixed_rows(pool, reg, lambda i, buf, n, exp: pool.spawn(i, 0, buf, n, exp),
                          lambda i, buf, n: spawn_without_row(pool, i, buf, n), lambda b: hashlib.sha1(b).digest())
        got = {r.index: r for r in pool.try_iter()}
        st = pool.stats()
        pool.unregister_buffer(reg)
    check_mixed(got, want, st)


def test_v2_slot_with_some_expected_rows(built, gpu):
    """The same slots of v2 pieces (32-byte rows, trees of 4 leaf slots); the
    count is 5 for the same reason."""
    from vortex_amd.hash_pool import HashPool

    reg = mmap.mmap(-1, 11 * STRIDE)
    with HashPool(PLEN, slots=2, batch_pieces=8) as pool:
        pool.register_buffer(reg)
        want = mixed_rows(pool, reg, lambda i, buf, n, exp: pool.spawn_merkle(i, 0, buf, n, exp),
                          lambda i, buf, n: pool.spawn_merkle(i, 0, buf, n, None), lambda b: hybrid.v2_root(b, 2))
        assert pool.try_iter() == []
        got = {r.index: r for r in pool.try_iter_merkle()}
        st = pool.stats()
        pool.unregister_buffer(reg)
    check_mixed(got, want, st)


def test_hybrid_piece_leaves_the_slot_when_its_launch_fails(built, gpu):
    """The first launch, the one the 8th submit triggers, fails (injected, host
    side only): that submit returns the error and its piece is not taken, the
    seven before it stay pending and are the unfinished ones; a new context
    takes hybrid pieces again."""
    from vortex_amd._lib import VX_EDEVICE, VxError
    from vortex_amd.hash_pool import HashPool

    lens = [32 * KiB - 7 * i for i in range(8)]
    bodies = [random_bytes(90 + i, L) for i, L in enumerate(lens)]
    pads = [32 * KiB - L for L in lens]
    sha1 = [hybrid.v1_digest(b, p) for b, p in zip(bodies, pads)]
    roots = [hybrid.v2_root(b, 1) for b in bodies]
    pool = HashPool(32 * KiB, slots=2, batch_pieces=8, hooks=True)
    pool.lib.vx_tuning_fail_launch_after(pool._h, 0)
    for i in range(7):
        pool.spawn_hybrid(i, 0, bodies[i], lens[i], pads[i], sha1[i], roots[i])
    with pytest.raises(VxError) as e:
        pool.spawn_hybrid(7, 0, bodies[7], lens[7], pads[7], sha1[7], roots[7])
    assert e.value.code == VX_EDEVICE and e.value.refused[0] == 7
    assert pool.pending == 7
    with pytest.raises(VxError):
        pool.try_iter_hybrid()
    assert sorted(i for i, _, _ in pool.take_unfinished()) == list(range(7))
    pool.close()
    with HashPool(32 * KiB, slots=2, batch_pieces=8) as pool:
        for i in range(8):
            pool.spawn_hybrid(i, 0, bodies[i], lens[i], pads[i], sha1[i], roots[i])
        pool.drain()
        got = {r.index: r for r in pool.try_iter_hybrid()}
        assert pool.pending == 0 and pool.stats()["batches"] == 1
    assert sorted(got) == list(range(8))
    assert all(got[i].matched == 3 and got[i].sha1 == sha1[i] and got[i].root == roots[i] for i in range(8))
