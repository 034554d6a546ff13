"""The runs of the merkle sweep's GPU files (test_gpu_merkle_leaf_sweep.py,
test_gpu_merkle_tree_sweep.py): each entry of vortex_amd.device on a batch of
pieces whose leaf rows and roots are known, with the files' rules built in.
Outputs are prefilled with 0xFF and carry one spare row or word that must stay
0xFF; inputs are compared with the host's after the call; `expected` is the
true table but for every third row, which is one bit away; a batch runs on
each buffer it is given and the runs must agree.  torch is imported by the
caller and handed in."""
import numpy as np

import _merkle_sweep as sw

FILL = 0xFF


def full(torch, gpu, shape, dtype=None):
    return torch.full(shape, FILL if dtype is None else -1, dtype=dtype or torch.uint8, device=gpu)


def rows(got, want, what, name=lambda k: f"row {k}"):
    """got [n + 1, 32] against want [n, 32] and the spare row."""
    n = len(want)
    got = got.cpu().numpy().reshape(-1, 32)
    bad = np.flatnonzero((got[:n] != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {n} rows differ from hashlib, first: {name(bad[0])}"
    assert (got[n:] == FILL).all(), f"{what}: a row behind the last was written"
    return got[:n]


def verdicts(matched, ok, what):
    n = len(ok)
    m = matched.cpu().numpy()
    bad = np.flatnonzero(m[:n] != ok)
    assert bad.size == 0, f"{what}: {bad.size} verdicts wrong, first: piece {bad[0]} reads {m[bad[0]]}"
    assert (m[n:] == FILL).all(), f"{what}: a verdict behind the last was written"


def bitmap(n, K, bad_rows):
    """The words merkle_block_check writes for n pieces of 2^K slots."""
    wpp = max(1, (1 << K) // 64)
    words = np.zeros(n * wpp, dtype=np.uint64)
    for g in bad_rows:
        i, b = g >> K, g & ((1 << K) - 1)
        words[i * wpp + (b >> 6)] |= np.uint64(1) << np.uint64(b & 63)
    return words


def rows_off(true):
    """(expected, rows that differ): every third row one bit away, in 32-bit word k % 8."""
    exp = true.copy()
    idx = np.arange(0, len(true), 3)
    exp[idx, 4 * (idx % 8) + (idx // 8) % 4] ^= (1 << (idx % 8)).astype(np.uint8)
    assert ((exp != true).any(axis=1).nonzero()[0] == idx).all()
    return exp, idx


def buffers(torch, gpu, host, flipped):
    out = [("as laid out", host)]
    if flipped is not None:
        out.append(("outside bytes inverted", flipped))
    return [(label, arr, torch.from_numpy(arr).to(gpu)) for label, arr in out]


def same(runs, what):
    if len(runs) == 2:
        assert np.array_equal(runs[0], runs[1]), f"{what}: the two buffers disagree"


def tables(torch, gpu, offs, lens):
    return torch.tensor(offs, dtype=torch.int64, device=gpu), torch.tensor(lens, dtype=torch.int32, device=gpu)


def unchanged(pairs, what):
    for t, arr in pairs:
        assert np.array_equal(t.cpu().numpy(), np.asarray(arr).astype(t.cpu().numpy().dtype)), \
            f"{what}: an input was modified"


# ---------------------------------------------------------------------------
# the entries, each on a batch of pieces (width K) with leaf rows and roots known
# ---------------------------------------------------------------------------
def ragged(torch, gpu, K, offs, lens, bufs, leaves, roots, lw=None, what="merkle_ragged"):
    from vortex_amd import device as vdev

    n = len(lens)
    d_offs, d_lens = tables(torch, gpu, offs, lens)
    d_lw = torch.tensor(lw, dtype=torch.uint8, device=gpu) if lw is not None else None
    exp_h, ok = sw.one_bit_off(roots)
    exp = torch.from_numpy(exp_h).to(gpu)
    runs = []
    for label, arr, data in bufs:
        out_l, out_r, out_m = full(torch, gpu, ((n << K) + 1, 32)), full(torch, gpu, (n + 1, 32)), full(torch, gpu, (n + 1,))
        vdev.merkle_ragged(data, d_offs, d_lens, K, log2w=d_lw, expected=exp, leaves=out_l, roots=out_r, matched=out_m)
        torch.cuda.synchronize()
        w = f"{what}, log2_width {K}, {label}"
        rows(out_l, leaves, w + ", leaves", lambda k: f"piece {k >> K} ({lens[k >> K]} bytes) slot {k & ((1 << K) - 1)}")
        runs.append(rows(out_r, roots, w + ", roots", lambda k: f"piece {k} ({lens[k]} bytes)"))
        verdicts(out_m, ok, w)
        unchanged([(data, arr), (d_offs, offs), (d_lens, lens), (exp, exp_h)], w)
    same(runs, what)


def pieces(torch, gpu, K, offs, lens, bufs, roots, lw=None, what="merkle_pieces"):
    from vortex_amd import device as vdev

    n = len(lens)
    d_offs, d_lens = tables(torch, gpu, offs, lens)
    d_lw = torch.tensor(lw, dtype=torch.uint8, device=gpu) if lw is not None else None
    exp_h, ok = sw.one_bit_off(roots)
    exp = torch.from_numpy(exp_h).to(gpu)
    runs = []
    for label, arr, data in bufs:
        out_r, out_m = full(torch, gpu, (n + 1, 32)), full(torch, gpu, (n + 1,))
        vdev.merkle_pieces(data, d_offs, d_lens, K, log2w=d_lw, expected=exp, roots=out_r, matched=out_m)
        torch.cuda.synchronize()
        w = f"{what}, log2_width {K}, log2w {'given' if lw is not None else 'absent'}, {label}"
        runs.append(rows(out_r, roots, w, lambda k: f"piece {k} ({lens[k]} bytes)"))
        verdicts(out_m, ok, w)
        unchanged([(data, arr), (d_offs, offs), (d_lens, lens), (exp, exp_h)], w)
    same(runs, what)


def block_check(torch, gpu, K, offs, lens, bufs, leaves):
    """Three forms: leaves only; the bitmap against the true rows (all zero);
    bitmap and leaves against rows of which every third is one bit off
    (exactly those blocks, but never a slot past its piece's end)."""
    from vortex_amd import device as vdev

    n, nrows = len(lens), len(leaves)
    W = 1 << K
    words = n * max(1, W // 64)
    d_offs, d_lens = tables(torch, gpu, offs, lens)
    off_h, idx = rows_off(leaves)
    live = [g for g in idx if (g & (W - 1)) * sw.LEAF < lens[g >> K]]
    assert 0 < len(live) and (K or len(live) < len(idx))  # (width 0: the empty pieces' rows are off too)
    want_bad = bitmap(n, K, live)
    true_d, off_d = torch.from_numpy(leaves).to(gpu), torch.from_numpy(off_h).to(gpu)
    name = lambda k: f"piece {k >> K} ({lens[k >> K]} bytes) slot {k & (W - 1)}"
    runs = []
    for label, arr, data in bufs:
        w = f"merkle_block_check, log2_width {K}, {label}"
        out_l = full(torch, gpu, (nrows + 1, 32))
        bad, got = vdev.merkle_block_check(data, d_offs, d_lens, K, leaves=out_l)
        torch.cuda.synchronize()
        assert bad is None and got is out_l
        runs.append(rows(out_l, leaves, w + ", leaves only", name))

        out_b = full(torch, gpu, (words + 1,), torch.int64)
        bad, got = vdev.merkle_block_check(data, d_offs, d_lens, K, expected_leaves=true_d, bad=out_b)
        torch.cuda.synchronize()
        b = out_b.cpu().numpy().view(np.uint64)
        assert got is None and not b[:words].any(), f"{w}: {np.count_nonzero(b[:words])} words set against the true rows"
        assert b[words] == np.uint64(0xFFFFFFFFFFFFFFFF), f"{w}: the spare word was written"

        out_b, out_l = full(torch, gpu, (words + 1,), torch.int64), full(torch, gpu, (nrows + 1, 32))
        vdev.merkle_block_check(data, d_offs, d_lens, K, expected_leaves=off_d, bad=out_b, leaves=out_l)
        torch.cuda.synchronize()
        b = out_b.cpu().numpy().view(np.uint64)
        wrong = np.flatnonzero(b[:words] != want_bad)
        assert wrong.size == 0, (f"{w}: {wrong.size} bitmap words wrong, first: word {wrong[0]} reads "
                                 f"{int(b[wrong[0]]):#x}, not {int(want_bad[wrong[0]]):#x}")
        assert b[words] == np.uint64(0xFFFFFFFFFFFFFFFF), f"{w}: the spare word was written"
        rows(out_l, leaves, w + ", leaves beside the bitmap", name)
        unchanged([(data, arr), (d_offs, offs), (d_lens, lens), (true_d, leaves), (off_d, off_h)], w)
    same(runs, "merkle_block_check")
