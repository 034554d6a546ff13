"""GPU: the SHA-1 kernels at the edges of their own loops, against hashlib.

The shapes come from tests/_sha1_sweep.py (derived from the ring depths in
the kernel sources; tests/test_sha1_sweep_cpu.py shows that they reach every
trip count, remainder and branch of every kernel).  Every digest is compared
bit-exactly with hashlib.sha1 of the same host bytes.  Rules of this file:

  * one random host array per batch, the pieces at 16-byte aligned offsets
    inside it, so the bytes around every piece are random, never zero;
  * output tensors have one spare row and are prefilled with 0xA5; the spare
    digest row and the spare verdict byte must still be 0xA5 afterwards;
  * `expected` holds the true digests, except that every 7th piece differs in
    exactly one bit, bit i % 8 of byte i % 20: those pieces, and only those,
    must read matched == 0 (a compare that dropped a word would pass them).

A disagreement between a producer's and a consumer's barrier counts would
show as a hang, not as a wrong digest: if this file hangs, read the code.
"""
import hashlib

import numpy as np
import pytest

import _sha1_sweep as sw

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_cache = {}


def _hash_rows(host, offs, lens):
    return np.frombuffer(b"".join(hashlib.sha1(host[o:o + L]).digest() for o, L in zip(offs, lens)),
                         dtype=np.uint8).reshape(len(lens), 20)


def _one_bit_off(want):
    """(expected, matched): every 7th row one bit away from the true digest."""
    exp = want.copy()
    idx = np.arange(0, len(want), 7)
    exp[idx, idx % 20] ^= (1 << (idx % 8)).astype(np.uint8)
    ok = np.ones(len(want), dtype=np.uint8)
    ok[idx] = 0
    return exp, ok


def _batch(name):
    """(host bytes, offsets, lengths, hashlib digests) of a ragged batch, built
    once; the host array is never modified."""
    if name not in _cache:
        lens = {"waves64": lambda: sw.batch_waves(sw.WAVE), "waves32": lambda: sw.batch_waves(sw.kZcPieces),
                "shuffled": sw.batch_s, "one": lambda: [64 * sw.kZcTileBlocks + 57]}[name]()
        offs, size = sw.layout(lens, gap=16)
        host = np.random.default_rng(len(lens)).integers(0, 256, size + 64, dtype=np.uint8)
        view = memoryview(host)
        _cache[name] = (host, offs, lens, _hash_rows(view, offs, lens))
    return _cache[name]


def _outputs(torch, gpu, n):
    return (torch.full((n + 1, 20), SENTINEL, dtype=torch.uint8, device=gpu),
            torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device=gpu))


def _compare(dig, matched, want, ok, lens, what):
    """dig [n+1, 20], matched [n+1] (device) against hashlib and the verdicts."""
    n = len(want)
    got, m = dig.cpu().numpy(), matched.cpu().numpy()
    bad = np.flatnonzero((got[:n] != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} digests differ from hashlib, first: piece {bad[0]} ({lens[bad[0]]} bytes)"
    bad = np.flatnonzero(m[:n] != ok)
    assert bad.size == 0, f"{what}: {bad.size} verdicts wrong, first: piece {bad[0]} reads {m[bad[0]]}"
    assert (got[n] == SENTINEL).all() and m[n] == SENTINEL, f"{what}: the spare output row was written"


# ---------------------------------------------------------------------------
# Uniform kernels: every length of the grid, n = 65 (one full wave and one lane)
# ---------------------------------------------------------------------------
UNIFORM_N = 65


def _uniform_stride(k, L):
    return (L + 15) // 16 * 16 + (16 if k % 2 == 0 else 48)


def _uniform_reference():
    """(host buffer, want [len(GRID), 65, 20]): piece i of length GRID[k] is
    host[i * stride_k : i * stride_k + GRID[k]], all in one shared buffer."""
    if "uniform" not in _cache:
        size = (UNIFORM_N - 1) * max(_uniform_stride(k, L) for k, L in enumerate(sw.GRID)) + max(sw.GRID) + 64
        host = np.random.default_rng(65).integers(0, 256, size, dtype=np.uint8)
        view = memoryview(host)
        want = np.stack([_hash_rows(view, [i * _uniform_stride(k, L) for i in range(UNIFORM_N)], [L] * UNIFORM_N)
                         for k, L in enumerate(sw.GRID)])
        _cache["uniform"] = (host, want)
    return _cache["uniform"]


def _uniform_sweep(gpu, variant, picks):
    import torch

    from vortex_amd import device as vdev

    host, want_all = _uniform_reference()
    data = torch.from_numpy(host).to(gpu)
    n, g = UNIFORM_N, len(picks)
    want = want_all[picks]
    exp_rows, ok_rows = zip(*(_one_bit_off(w) for w in want))
    exp = torch.from_numpy(np.stack(exp_rows)).to(gpu)
    dig = torch.full((g, n + 1, 20), SENTINEL, dtype=torch.uint8, device=gpu)
    matched = torch.full((g, n + 1), SENTINEL, dtype=torch.uint8, device=gpu)
    for j, k in enumerate(picks):
        L = sw.GRID[k]
        vdev.sha1_uniform(data, n, L, stride=_uniform_stride(k, L), expected=exp[j], digests=dig[j],
                          matched=matched[j], variant=variant)
    torch.cuda.synchronize()
    for j, k in enumerate(picks):
        _compare(dig[j], matched[j], want[j], ok_rows[j], [sw.GRID[k]] * n, f"variant {variant}, length {sw.GRID[k]}")


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_uniform_grid(built, gpu, variant):
    _uniform_sweep(gpu, variant, list(range(len(sw.GRID))))


def test_uniform_default_dispatch(built, gpu):
    """Variant 0 is one of these kernels: a tenth of the grid through
    vx_sha1_device_uniform."""
    _uniform_sweep(gpu, 0, list(range(0, len(sw.GRID), 10)))


# ---------------------------------------------------------------------------
# Ragged kernels: the wave recipes and the shuffled grid, in three lane orders
# ---------------------------------------------------------------------------
def _orders(torch, gpu, lens):
    from vortex_amd import device as vdev

    perm = np.random.default_rng(len(lens) + 1).permutation(len(lens)).astype(np.int32)
    return (("lane order", None), ("length order", vdev.length_order(lens).to(gpu)),
            ("a random permutation", torch.from_numpy(perm).to(gpu)))


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
def test_ragged_recipes(built, gpu, variant):
    """Variant 0 goes through the planner (plan=ragged_plan(lens)).  A sorted
    order alone never tests `order` as an indirection, hence the permutation."""
    import torch

    from vortex_amd import device as vdev

    for name in ("waves64", "shuffled"):
        host, offs, lens, want = _batch(name)
        n = len(lens)
        data = torch.from_numpy(host).to(gpu)
        d_offs = torch.tensor(offs, dtype=torch.int64, device=gpu)
        d_lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
        exp_h, ok = _one_bit_off(want)
        exp = torch.from_numpy(exp_h).to(gpu)
        plan = vdev.ragged_plan(lens) if variant == 0 else None
        for label, order in _orders(torch, gpu, lens):
            dig, matched = _outputs(torch, gpu, n)
            vdev.sha1_ragged(data, d_offs, d_lens, order=order, expected=exp, digests=dig, matched=matched,
                             variant=variant, plan=plan)
            torch.cuda.synchronize()
            _compare(dig, matched, want, ok, lens, f"variant {variant}, {name} in {label}")


# ---------------------------------------------------------------------------
# The zero-copy kernel on its own, its sources in HBM
# ---------------------------------------------------------------------------
def _zero_copy(torch, gpu, data, d_offs, d_lens, n, dig, exp, matched, loader):
    from vortex_amd._lib import check, tuning

    srcs = d_offs + data.data_ptr()  # device-visible addresses, 16-byte aligned
    check(tuning().vx_tuning_zero_copy_kernel(srcs.data_ptr(), d_lens.data_ptr(), n, dig.data_ptr(),
                                              exp.data_ptr() if exp is not None else None,
                                              matched.data_ptr() if exp is not None else None, loader,
                                              int(torch.cuda.current_stream(gpu).cuda_stream)),
          "vx_tuning_zero_copy_kernel", tuning())
    torch.cuda.synchronize()


@pytest.mark.parametrize("loader", [0, 1])
def test_zero_copy_recipes(built, gpu, loader):
    """The recipes in their 32-piece form (n = 1 mod 32), the shuffled grid
    (n = 27 mod 32) and a batch of one piece; the pair and the three-wave form."""
    import torch

    for name in ("waves32", "shuffled", "one"):
        host, offs, lens, want = _batch(name)
        n = len(lens)
        assert n % sw.kZcPieces
        data = torch.from_numpy(host).to(gpu)
        d_offs = torch.tensor(offs, dtype=torch.int64, device=gpu)
        d_lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
        exp_h, ok = _one_bit_off(want)
        dig, matched = _outputs(torch, gpu, n)
        _zero_copy(torch, gpu, data, d_offs, d_lens, n, dig, torch.from_numpy(exp_h).to(gpu), matched, loader)
        _compare(dig, matched, want, ok, lens, f"zero-copy loader {loader}, {name}")


# ---------------------------------------------------------------------------
# Bytes outside the pieces do not matter
# ---------------------------------------------------------------------------
def _outside_flipped(host, offs, lens):
    """A copy of host with every byte outside the pieces XORed with 0xFF."""
    delta = np.zeros(len(host) + 1, dtype=np.int32)
    np.add.at(delta, np.asarray(offs, dtype=np.int64), 1)
    np.add.at(delta, np.asarray(offs, dtype=np.int64) + np.asarray(lens, dtype=np.int64), -1)
    inside = np.cumsum(delta[:-1]) > 0
    out = host.copy()
    out[~inside] ^= 0xFF
    assert (out[inside] == host[inside]).all() and (out != host).sum() == (~inside).sum() > 0
    return out


@pytest.mark.parametrize("family", ["ragged 1", "ragged 2", "zero-copy 0", "zero-copy 1"])
def test_outside_bytes_do_not_matter_ragged(built, gpu, family):
    """The recipe batch twice: as laid out, and with every byte outside the
    pieces inverted.  Both runs give hashlib's digests."""
    import torch

    from vortex_amd import device as vdev

    kind, arg = family.rsplit(" ", 1)
    host, offs, lens, want = _batch("waves64" if kind == "ragged" else "waves32")
    n = len(lens)
    d_offs = torch.tensor(offs, dtype=torch.int64, device=gpu)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
    exp_h, ok = _one_bit_off(want)
    exp = torch.from_numpy(exp_h).to(gpu)
    runs = []
    for label, src in (("as laid out", host), ("outside bytes inverted", _outside_flipped(host, offs, lens))):
        data = torch.from_numpy(src).to(gpu)
        dig, matched = _outputs(torch, gpu, n)
        if kind == "ragged":
            vdev.sha1_ragged(data, d_offs, d_lens, expected=exp, digests=dig, matched=matched, variant=int(arg))
            torch.cuda.synchronize()
        else:
            _zero_copy(torch, gpu, data, d_offs, d_lens, n, dig, exp, matched, int(arg))
        _compare(dig, matched, want, ok, lens, f"{family}, {label}")
        runs.append(dig.cpu())
    assert torch.equal(runs[0], runs[1])


def test_outside_bytes_do_not_matter_uniform(built, gpu):
    """The default uniform kernel on a tenth of the grid, each length with the
    bytes between its pieces inverted."""
    import torch

    from vortex_amd import device as vdev

    host, want_all = _uniform_reference()
    n = UNIFORM_N
    clean = torch.from_numpy(host).to(gpu)
    for k in range(3, len(sw.GRID), 10):
        L, stride = sw.GRID[k], _uniform_stride(k, sw.GRID[k])
        exp_h, ok = _one_bit_off(want_all[k])
        exp = torch.from_numpy(exp_h).to(gpu)
        flipped = torch.from_numpy(_outside_flipped(host, [i * stride for i in range(n)], [L] * n)).to(gpu)
        runs = []
        for label, data in (("as laid out", clean), ("outside bytes inverted", flipped)):
            dig, matched = _outputs(torch, gpu, n)
            vdev.sha1_uniform(data, n, L, stride=stride, expected=exp, digests=dig, matched=matched)
            runs.append((dig, matched, label))
        torch.cuda.synchronize()
        for dig, matched, label in runs:
            _compare(dig, matched, want_all[k], ok, [L] * n, f"uniform default, length {L}, {label}")
        assert torch.equal(runs[0][0], runs[1][0])
