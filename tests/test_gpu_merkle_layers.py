"""GPU: v2 `piece layers` and hash proofs in batches (vx_merkle_device_layers,
vx_merkle_device_proofs, vx_merkle_verify_layers, vx_merkle_verify_proofs)
against hashlib, bit-exact.  Every output tensor the tests own is filled with
0xFF and has one spare row that must stay 0xFF; inputs are compared with
themselves after the call."""
import ctypes
import hashlib
import random

import pytest

from test_merkle_layers_cpu import COUNTS, _pad, _sha, model_root, walk

pytestmark = pytest.mark.gpu
KiB = 1024


def _dev_rows(blob, dev):
    import torch

    return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev).view(-1, 32)


def _ff(rows, dev, width=32):
    import torch

    shape = (rows, width) if width else (rows,)
    return torch.full(shape, 0xFF, dtype=torch.uint8, device=dev)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _split(blob, counts):
    out, at = [], 0
    for c in counts:
        out.append([blob[32 * k:32 * k + 32] for k in range(at, at + c)])
        at += c
    return out


@pytest.fixture(scope="module")
def big():
    """The count list's input and its hashlib roots at both heights (computed once)."""
    blob = random.Random(0x1A7E25).randbytes(32 * sum(COUNTS))
    layers = _split(blob, COUNTS)
    return blob, {h: [model_root(rows, h) for rows in layers] for h in (0, 4)}


# ---- layers --------------------------------------------------------------------

@pytest.mark.parametrize("height", [0, 4])
def test_count_list_in_one_call(built, gpu, big, height):
    import torch

    from vortex_amd import device as vdev

    blob, want = big
    n = len(COUNTS)
    hashes = _dev_rows(blob, gpu)
    exp = [bytearray(r) for r in want[height]]
    for f in range(0, n, 3):  # every third root one bit off, a different byte per layer
        exp[f][f % 32] ^= 1 << (f % 8)
    expected = _dev_rows(b"".join(exp), gpu)
    roots, matched = _ff(n + 1, gpu), _ff(n + 1, gpu, 0)
    got_roots, got_matched = vdev.merkle_layers(hashes, COUNTS, height, expected=expected, roots=roots,
                                                matched=matched)
    torch.cuda.synchronize()
    assert got_roots is roots and got_matched is matched
    raw = _bytes(roots)
    for f in range(n):
        assert raw[32 * f:32 * f + 32] == want[height][f], f"layer {f} of {COUNTS[f]} hashes"
    assert raw[32 * n:] == b"\xFF" * 32
    assert _bytes(matched) == bytes(0 if f % 3 == 0 else 1 for f in range(n)) + b"\xFF"
    assert _bytes(hashes) == blob and _bytes(expected) == b"".join(exp)
    # ... and the one-layer entry agrees, layer by layer
    at = 0
    for f, c in enumerate(COUNTS):
        one = vdev.merkle_root(hashes[at:at + c], height)
        assert _bytes(one) == want[height][f], f"merkle_root, layer {f}"
        at += c


def test_three_thousand_small_layers(built, gpu):
    import torch

    from vortex_amd import device as vdev

    counts = [2 + i % 8 for i in range(3000)]
    blob = random.Random(3000).randbytes(32 * sum(counts))
    want = [model_root(rows, 2) for rows in _split(blob, counts)]
    hashes = _dev_rows(blob, gpu)
    roots = _ff(len(counts) + 1, gpu)
    vdev.merkle_layers(hashes, counts, 2, roots=roots)
    torch.cuda.synchronize()
    assert _bytes(roots) == b"".join(want) + b"\xFF" * 32
    assert _bytes(hashes) == blob


def test_verdicts_only_and_no_layers(built, gpu):
    import torch

    from vortex_amd import device as vdev

    counts = [5, 513, 1, 64]
    blob = random.Random(5).randbytes(32 * sum(counts))
    want = [model_root(rows, 1) for rows in _split(blob, counts)]
    want[1] = bytes(32)
    hashes, expected = _dev_rows(blob, gpu), _dev_rows(b"".join(want), gpu)
    matched = _ff(len(counts) + 1, gpu, 0)
    roots, got = vdev.merkle_layers(hashes, counts, 1, expected=expected, matched=matched)
    torch.cuda.synchronize()
    assert roots is None and got is matched
    assert _bytes(matched) == bytes([1, 0, 1, 1]) + b"\xFF"
    assert _bytes(hashes) == blob
    # no layers: nothing is launched, nothing is written
    none = torch.empty((0, 32), dtype=torch.uint8, device=gpu)
    roots, matched = _ff(1, gpu), _ff(1, gpu, 0)
    vdev.merkle_layers(none, [], 3, expected=none, roots=roots, matched=matched)
    torch.cuda.synchronize()
    assert _bytes(roots) == b"\xFF" * 32 and _bytes(matched) == b"\xFF"
    r0, m0 = vdev.merkle_layers(none, [], 3)
    assert tuple(r0.shape) == (0, 32) and m0 is None
    with pytest.raises(ValueError):
        vdev.merkle_layers(hashes, [5, 513, 1, 63], 1)  # the rows do not add up
    with pytest.raises(Exception):
        vdev.merkle_layers(hashes, [5, 513, 0, 65], 1)  # a zero count


# ---- proofs ----------------------------------------------------------------------

HEIGHT = 3


@pytest.fixture(scope="module")
def batch():
    """One batch of proofs over a layer of 1,000 hashes at height 3 (1,024 after
    padding): for every span the first, the last and a middle one, each proved
    to the root and, with half its uncles, to a trusted ancestor; a bare hash
    (span 1, no uncles); a synthetic chain of 40 uncles whose pos has bits
    above bit 32.  Returns (rows, proofs, expected rows, the walks' tops)."""
    from vortex_amd import merkle

    rng = random.Random(1000)
    layer = [rng.randbytes(32) for _ in range(1000)]
    rows, proofs, expected, tops = [], [], [model_root(layer, HEIGHT)], []

    def add(proof_rows, pos, span, uncles):
        top = walk(proof_rows, span, uncles, pos)
        if top not in expected:
            expected.append(top)
        proofs.append((pos, len(rows), expected.index(top), span, uncles))
        rows.extend(proof_rows[k:k + 32] for k in range(0, len(proof_rows), 32))
        tops.append(top)

    span = 1
    while span <= 512:
        spans = 1024 // span
        total = spans.bit_length() - 1
        for pos in sorted({0, spans - 1, spans // 2}):
            add(merkle.make_proof(layer, HEIGHT, pos, span, total), pos, span, total)
            assert proofs[-1][2] == 0  # ... reaches the root
            add(merkle.make_proof(layer, HEIGHT, pos, span, total // 2), pos, span, total // 2)
        span *= 2
    add(layer[17], 17, 1, 0)
    add(rng.randbytes(32 * (2 + 40)), (0xA5 << 32) | 0x01234567, 2, 40)
    assert proofs[-1][0] >> 33 and proofs[-1][4] == 40
    return rows, proofs, expected, tops


def _raw_proofs(gpu, rows, proof_array, n, expected):
    """vx_merkle_device_proofs itself, on tensors of the test's own."""
    import torch

    from vortex_amd import _lib

    hashes, exp = _dev_rows(b"".join(rows), gpu), _dev_rows(b"".join(expected), gpu)
    d_proofs = torch.frombuffer(bytearray(bytes(proof_array)), dtype=torch.uint8).to(gpu)
    tops, matched = _ff(n + 1, gpu), _ff(n + 1, gpu, 0)
    rc = _lib.lib().vx_merkle_device_proofs(hashes.data_ptr(), d_proofs.data_ptr(), n, tops.data_ptr(),
                                            exp.data_ptr(), matched.data_ptr(),
                                            int(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == 0, _lib.lib().vx_last_error()
    torch.cuda.synchronize()
    assert _bytes(hashes) == b"".join(rows) and _bytes(exp) == b"".join(expected)
    assert _bytes(d_proofs) == bytes(proof_array)
    t, m = _bytes(tops), _bytes(matched)
    assert t[32 * n:] == b"\xFF" * 32 and m[n:] == b"\xFF"
    return [t[32 * k:32 * k + 32] for k in range(n)], list(m[:n])


def test_proofs_bit_exact(built, gpu, batch):
    import torch

    from vortex_amd import _lib
    from vortex_amd import device as vdev

    rows, proofs, expected, want = batch
    n = len(proofs)
    hashes, exp = _dev_rows(b"".join(rows), gpu), _dev_rows(b"".join(expected), gpu)
    tops, matched = vdev.merkle_proofs(hashes, proofs, exp)
    torch.cuda.synchronize()
    got = _bytes(tops)
    for i in range(n):
        assert got[32 * i:32 * i + 32] == want[i], f"proof {i}: {proofs[i]}"
    assert _bytes(matched) == b"\x01" * n
    assert _bytes(hashes) == b"".join(rows) and _bytes(exp) == b"".join(expected)
    # the same through the raw entry, on guarded outputs
    assert _raw_proofs(gpu, rows, _lib.proof_array(proofs), n, expected) == (want, [1] * n)
    # the wrapper checks what the host entry checks
    for bad, word in (((0, 0, 0, 3, 1), "span"), ((0, 0, 0, 4, 65), "uncles"), ((0, len(rows) - 3, 0, 4, 0), "n_rows"),
                      ((0, 0, len(expected), 4, 0), "expected")):
        with pytest.raises(ValueError, match=word):
            vdev.merkle_proofs(hashes, proofs[:2] + [bad], exp)


def test_planted_faults_fail_exactly_their_proof(built, gpu, batch):
    from vortex_amd import _lib

    rows, proofs, expected, want = batch
    n = len(proofs)
    # victims that have what the fault needs: uncles to flip, a span of real
    # rows, and a sibling that differs from the running hash (real rows both)
    uncle_victim = next(i for i, p in enumerate(proofs) if p[3] == 8 and p[4] == 7)
    span_victim = next(i for i, p in enumerate(proofs) if p[3] == 64 and p[0] == 0 and p[4] == 2)
    pos_victim = next(i for i, p in enumerate(proofs) if p[3] == 4 and p[0] == 0 and p[4] == 8)
    for victim, what in ((uncle_victim, "uncle"), (span_victim, "span"), (pos_victim, "pos")):
        r, p = list(rows), list(proofs)
        pos, row, e, span, uncles = p[victim]
        if what == "uncle":
            at = row + span + uncles - 1  # the last uncle
            r[at] = r[at][:31] + bytes([r[at][31] ^ 0x80])
        elif what == "span":
            at = row + span // 2
            r[at] = bytes([r[at][0] ^ 1]) + r[at][1:]
        else:
            p[victim] = (pos ^ 1, row, e, span, uncles)
        tops, matched = _raw_proofs(gpu, r, _lib.proof_array(p), n, expected)
        assert matched == [0 if i == victim else 1 for i in range(n)], what
        assert [i for i in range(n) if tops[i] != want[i]] == [victim], what
        assert tops[victim] == walk(b"".join(r[row:row + span + uncles]), span, uncles, p[victim][0])


@pytest.mark.parametrize("fill", [0xFF, 0x5A])
def test_bad_descriptors_read_nothing(built, gpu, fill):
    """span 3, span 1024 and uncles 65 straight to the device entry: matched 0,
    a zero top, and the rows such a proof names stay unread, so the result is
    the same whatever they hold."""
    from vortex_amd import _lib, merkle

    rng = random.Random(65)
    layer = [rng.randbytes(32) for _ in range(16)]
    good = merkle.make_proof(layer, 0, 5, 2, 3)
    good_rows = [good[k:k + 32] for k in range(0, len(good), 32)]
    guard = [bytes([fill]) * 32] * (1024 + 65)
    rows = good_rows + guard + good_rows
    g0, g1 = 0, len(good_rows) + len(guard)
    root = model_root(layer, 0)
    arr = (_lib.vx_merkle_proof * 6)()
    for k, (pos, row, span, uncles) in enumerate([(5, g0, 2, 3), (0, len(good_rows), 3, 2), (5, g1, 2, 3),
                                                  (0, len(good_rows), 1024, 0), (1, len(good_rows), 4, 65),
                                                  (5, g0, 2, 3)]):
        arr[k].pos, arr[k].row, arr[k].expected, arr[k].span, arr[k].uncles = pos, row, 0, span, uncles
    tops, matched = _raw_proofs(gpu, rows, arr, 6, [root, bytes(32)])
    assert matched == [1, 0, 1, 0, 0, 1]
    assert tops == [root, bytes(32), root, bytes(32), bytes(32), root]
    for k in (1, 3, 4):  # with the zero row itself as the expected one, a zero top must still not match
        arr[k].expected = 1
    tops, matched = _raw_proofs(gpu, rows, arr, 6, [root, bytes(32)])
    assert matched == [1, 0, 1, 0, 0, 1] and tops == [root, bytes(32), root, bytes(32), bytes(32), root]


# ---- host entries on a context -----------------------------------------------------

def _piece_root(body, lw):
    rows = [hashlib.sha256(body[o:o + 16384]).digest() if o < len(body) else bytes(32)
            for o in range(0, 16384 << lw, 16384)]
    while len(rows) > 1:
        rows = [_sha(rows[k], rows[k + 1]) for k in range(0, len(rows), 2)]
    return rows[0]


def test_verify_piece_layers(built, gpu):
    from vortex_amd.hash_pool import HashPool

    rng = random.Random(52)
    pl = 64 * KiB  # pieces of 4 blocks: the layers stand 2 levels above the leaves
    layers = [rng.randbytes(32 * c) for c in (2, 700, 5)]
    roots = [model_root(_split(x, [len(x) // 32])[0], 2) for x in layers]
    assert roots[0] == _sha(layers[0][:32], layers[0][32:]) and _pad(2) != bytes(32)
    with HashPool(pl, slots=2, batch_pieces=8) as pool:
        assert pool.verify_piece_layers(layers, roots, pl) == [True, True, True]
        wrong = [roots[0], bytes([roots[1][0] ^ 1]) + roots[1][1:], roots[2]]
        assert pool.verify_piece_layers(layers, wrong, pl) == [True, False, True]
        # at another piece length the padding differs: the layers that need padding fail
        assert pool.verify_piece_layers(layers, roots, 32 * KiB) == [True, False, False]
        assert pool.verify_piece_layers([], [], pl) == []
        assert pool.stats()["pieces_completed"] == 0 and pool.stats()["batches"] == 0


def test_proofs_while_a_piece_is_pending(built, gpu, batch):
    """Proofs for one file arrive while another file's pieces download: the
    call works with a v2 piece queued and unflushed, the piece's completion
    still arrives, and stats() is what it would have been without the call."""
    from vortex_amd import _lib
    from vortex_amd.hash_pool import HashPool

    rows, proofs, expected, _ = batch
    body = random.Random(9).randbytes(40000)
    root = _piece_root(body, 2)
    steady = ("pieces_completed", "pieces_mismatched", "bytes_completed", "batches", "chunk_rounds", "gather_tiles",
              "staged_bytes", "io_errors", "batch_latency_count", "zero_copy_slots", "zero_copy_loader_slots",
              "submits_refused")
    seen = []
    for with_call in (False, True):
        with HashPool(64 * KiB, slots=2, batch_pieces=8) as pool:
            pool.spawn_merkle(7, 1, body, len(body), root)
            assert pool.pending == 1
            if with_call:
                before = pool.stats()
                assert pool.verify_hash_proofs(b"".join(rows), proofs, expected) == [True] * len(proofs)
                flipped = list(expected)
                flipped[0] = bytes(32)
                assert pool.verify_hash_proofs(b"".join(rows), proofs, flipped) == [p[2] != 0 for p in proofs]
                with pytest.raises(_lib.VxError, match="proof 1: span") as err:
                    pool.verify_hash_proofs(b"".join(rows), [proofs[0], (0, 0, 0, 6, 0)], expected)
                assert err.value.code == _lib.VX_EINVAL
                assert pool.verify_hash_proofs(b"", [], []) == []
                assert pool.pending == 1 and pool.stats() == before
            pool.drain()
            done = pool.try_iter_merkle()
            assert [(r.index, r.hash_matched, r.digest) for r in done] == [(7, True, root)]
            st = pool.stats()
            seen.append({k: st[k] for k in steady})
    assert seen[0] == seen[1] and seen[0]["pieces_completed"] == 1
