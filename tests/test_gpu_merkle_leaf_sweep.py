"""GPU: the SHA-256 leaf lane at every length and in every kind of wave, through
each of its five entries, against hashlib.

The lane (leaf_len, ng, the wave-wide ring bound, stream_groups, finish_tail,
the zero hash) is written out in merkle_leaf_kernel<true> and <false>,
merkle_block_check_kernel, merkle_block_kernel and merkle_piece_kernel.  The
shapes come from tests/_merkle_sweep.py; tests/test_merkle_sweep_cpu.py shows
that every class of lane and wave is in the launches of every entry.  Every
row is compared bit-exactly with hashlib.sha256 of the same host bytes.  Rules
of this file:

  * pieces at 16-byte aligned offsets of one random host array, walking the
    eight phases of a 128-byte line, so the bytes around a piece are random;
  * every entry runs on that array and on a copy with every byte outside the
    pieces inverted: both give hashlib's rows;
  * outputs are prefilled with 0xFF and have one spare row or word that must
    still be 0xFF afterwards; inputs are compared with the host's after the call;
  * `expected` is the true table except for every third row, which is one bit
    away: those, and only those, read as a mismatch.
"""
import numpy as np
import pytest

import _merkle_sweep as sw
import _merkle_sweep_run as run

pytestmark = pytest.mark.gpu

FILL = run.FILL
_cache = {}


def _recipes():
    """(lens, offs, host, flipped, want [n, 32]) of the recipe batch, built once and never modified."""
    if "recipes" not in _cache:
        lens = sw.leaf_batch()
        offs, host, flipped = sw.layout(lens)
        _cache["recipes"] = (lens, offs, host, flipped, sw.hash_rows(host, offs, lens))
    return _cache["recipes"]


def _tails(K):
    """One piece per tail r at two groups, the short leaf in the last of 2^K slots."""
    if ("tails", K) not in _cache:
        lens = [((1 << K) - 1) * sw.LEAF + 256 + r for r in range(128)]
        _cache["tails", K] = sw.Pieces(K, [K] * len(lens), lens, overlapped=(K == 6))
    return _cache["tails", K]


# ---------------------------------------------------------------------------
# the wave recipes at log2_width 0: a piece is a leaf
# ---------------------------------------------------------------------------
def test_recipes_ragged(built, gpu):
    import torch

    lens, offs, host, flipped, want = _recipes()
    run.ragged(torch, gpu, 0, offs, lens, run.buffers(torch, gpu, host, flipped), want, want)


def test_recipes_pieces(built, gpu):
    import torch

    lens, offs, host, flipped, want = _recipes()
    bufs = run.buffers(torch, gpu, host, flipped)
    run.pieces(torch, gpu, 0, offs, lens, bufs, want)
    run.pieces(torch, gpu, 0, offs, lens, bufs, want, lw=[0] * len(lens))


def test_recipes_block_check(built, gpu):
    import torch

    lens, offs, host, flipped, want = _recipes()
    run.block_check(torch, gpu, 0, offs, lens, run.buffers(torch, gpu, host, flipped), want)


def test_recipes_blocks(built, gpu):
    """merkle_blocks: lane b is stage block b.  The batch goes in launches of
    at most 15 MiB of stage; rows in a permuted order, two rows skipped."""
    import torch

    from vortex_amd import device as vdev

    lens, offs, host, _, want = _recipes()
    for at, part, skipped in sw.blocks_launches(lens):
        m = len(part)
        stage, flipped = sw.stage_layout(host, offs[at:at + m], part, seed=at)
        perm = np.random.default_rng(at + 1).permutation(m).astype(np.int64)
        rows = perm.copy()
        rows[list(skipped)] = vdev.SKIP_ROW
        want_rows = np.full((m, 32), FILL, dtype=np.uint8)
        keep = np.array([k for k in range(m) if k not in skipped])
        want_rows[perm[keep]] = want[at + keep]  # the skipped lanes' rows stay as they were
        d_rows, d_lens = torch.from_numpy(rows).to(gpu), torch.tensor(part, dtype=torch.int32, device=gpu)
        runs = []
        for label, arr, data in run.buffers(torch, gpu, stage, flipped):
            out = run.full(torch, gpu, (m + 1, 32))
            vdev.merkle_blocks(data, d_rows, d_lens, out)
            torch.cuda.synchronize()
            w = f"merkle_blocks, lanes {at}..{at + m}, {label}"
            inv = {int(r): k for k, r in enumerate(perm)}
            runs.append(run.rows(out, want_rows, w, lambda r: f"row {r}, block {inv[r]} ({part[inv[r]]} bytes)"))
            run.unchanged([(data, arr), (d_rows, rows), (d_lens, part)], w)
        run.same(runs, "merkle_blocks")


# ---------------------------------------------------------------------------
# merkle_uniform (merkle_leaf_kernel<false>): one length a launch and a last piece of another
# ---------------------------------------------------------------------------
def test_uniform_grid(built, gpu):
    import torch

    from vortex_amd import device as vdev

    pairs = sw.uniform_pairs()
    size = max((n - 1) * sw.uniform_stride(a) + b for _, a, b, n in pairs) + 64
    host = sw.random_bytes(sw.SEED + 65, size)
    clean = torch.from_numpy(host).to(gpu)
    n_max = max(n for _, _, _, n in pairs)
    done = []
    for name, a, b, n in pairs:
        stride = sw.uniform_stride(a)
        offs, lens = [i * stride for i in range(n)], [a] * (n - 1) + [b]
        want = sw.hash_rows(host, offs, lens)
        exp_h, ok = sw.one_bit_off(want)
        exp = torch.from_numpy(exp_h).to(gpu)
        used = offs[-1] + b + 64
        flipped = torch.from_numpy(sw.outside_flipped(host[:used], offs, lens)).to(gpu)
        for label, data in (("as laid out", clean), ("outside bytes inverted", flipped)):
            out_l, out_r, out_m = run.full(torch, gpu, (n_max + 1, 32)), run.full(torch, gpu, (n_max + 1, 32)), run.full(torch, gpu, (n_max + 1,))
            vdev.merkle_uniform(data, n, a, 0, stride=stride, last_len=b, expected=exp, leaves=out_l, roots=out_r,
                                matched=out_m)
            done.append((f"merkle_uniform {name}: {n} pieces of {a} bytes, the last {b}, {label}", want, ok, out_l,
                         out_r, out_m))
    torch.cuda.synchronize()
    for k, (w, want, ok, out_l, out_r, out_m) in enumerate(done):
        got_l = run.rows(out_l, want, w + ", leaves", lambda i: f"piece {i}")
        run.rows(out_r, want, w + ", roots", lambda i: f"piece {i}")
        run.verdicts(out_m, ok, w)
        if k & 1:
            assert np.array_equal(got_l, done[k - 1][3].cpu().numpy()[:len(want)]), w
    assert np.array_equal(clean.cpu().numpy(), host), "merkle_uniform: the data was modified"


# ---------------------------------------------------------------------------
# the same tails in the last slot of a wider piece: slot 1 of 2, slot 63 of 64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log2_width", [1, 6])
def test_tails_in_the_last_slot(built, gpu, log2_width):
    """The short leaf sits on odd lanes (width 1) or on lane 63 of every wave
    and thread 255 of every fourth (width 6).  The pieces of width 6 share
    their bytes (128 pieces of a MiB each in one buffer of about a MiB)."""
    import torch

    K = log2_width
    p = _tails(K)
    assert sorted({(L & 127) for L in p.lens}) == list(range(128)) and all((L >> 7) % 128 == 2 for L in p.lens)
    bufs = run.buffers(torch, gpu, p.host, p.flipped)
    run.ragged(torch, gpu, K, p.offs, p.lens, bufs, p.leaves, p.roots)
    run.pieces(torch, gpu, K, p.offs, p.lens, bufs, p.roots)
    run.block_check(torch, gpu, K, p.offs, p.lens, bufs, p.leaves)
