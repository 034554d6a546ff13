"""GPU: the merkle tree reductions at every width, every per-piece width and every
position of a piece in its tile, against hashlib and the BEP 52 model.

merkle_node_kernel (trees of at most 512 leaves, through merkle_nodes) runs
alone on random rows at log2_width 0..9; merkle_piece_kernel's tree phase
(through merkle_pieces) at 0..10, the last two with the node launch that
follows it; the same buffers go through merkle_ragged, so the leaf + node pair
is compared at every width as well.  The shapes come from tests/_merkle_sweep.py:
max(2, K + 1) or more whole tiles and a lone piece in a last one, every width
0..K at the first and at the last position of a whole tile
(tests/test_merkle_sweep_cpu.py asserts it).  The rules are those of
test_gpu_merkle_leaf_sweep.py: outputs prefilled with 0xFF and one spare row,
inputs compared after the call, expected one bit off for every third piece.
"""
import numpy as np
import pytest

import _merkle_sweep as sw
import _merkle_sweep_run as run

pytestmark = pytest.mark.gpu

FILL = run.FILL
_cache = {}


def _batch(K):
    if K not in _cache:
        _cache[K] = sw.piece_batch(K)
    return _cache[K]


def _nodes_c(torch, leaves, lw, n, K, roots, expected, matched):
    """vx_merkle_device_nodes itself: the wrapper always passes a roots tensor."""
    from vortex_amd._lib import check, lib

    ptr = lambda t: t.data_ptr() if t is not None else None
    check(lib().vx_merkle_device_nodes(ptr(leaves), ptr(lw), n, K, ptr(roots), ptr(expected), ptr(matched),
                                       int(torch.cuda.current_stream(leaves.device).cuda_stream)),
          "vx_merkle_device_nodes")


# ---------------------------------------------------------------------------
# merkle_node_kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log2_width", range(sw.TILE_LOG2 + 1))
def test_nodes_width_shape(built, gpu, log2_width):
    """Random rows; the rows behind a piece's first 2^log2w do not matter."""
    import torch

    from vortex_amd import device as vdev

    K = log2_width
    lw = sw.tree_shape("node", K)
    n = len(lw)
    rows_h, flipped_h, roots = sw.node_rows(K, lw)
    exp_h, ok = sw.one_bit_off(roots)
    exp, d_lw = torch.from_numpy(exp_h).to(gpu), torch.tensor(lw, dtype=torch.uint8, device=gpu)
    name = lambda i: f"piece {i} (log2w {lw[i]}, position {i % sw.per_tile('node', K)} of tile {i // sw.per_tile('node', K)})"
    runs = []
    for label, arr in (("random rows", rows_h), ("rows outside the trees inverted", flipped_h)):
        w = f"merkle_nodes, log2_width {K}, {label}"
        leaves = torch.from_numpy(arr).to(gpu)
        out_r, out_m = run.full(torch, gpu, (n + 1, 32)), run.full(torch, gpu, (n + 1,))
        vdev.merkle_nodes(leaves, n, K, log2w=d_lw, expected=exp, roots=out_r, matched=out_m)
        only_r = run.full(torch, gpu, (n + 1, 32))
        _, none = vdev.merkle_nodes(leaves, n, K, log2w=d_lw, roots=only_r)
        only_m = run.full(torch, gpu, (n + 1,))
        _nodes_c(torch, leaves, d_lw, n, K, None, exp, only_m)
        torch.cuda.synchronize()
        assert none is None
        runs.append(run.rows(out_r, roots, w + ", roots and verdicts", name))
        run.verdicts(out_m, ok, w + ", roots and verdicts")
        run.rows(only_r, roots, w + ", roots only", name)
        run.verdicts(only_m, ok, w + ", verdicts only")
        run.unchanged([(leaves, arr), (d_lw, lw), (exp, exp_h)], w)
    run.same(runs, "merkle_nodes")


@pytest.mark.parametrize("log2_width", range(sw.TILE_LOG2 + 1))
def test_nodes_count_batches(built, gpu, log2_width):
    """n either side of a tile's piece count, every piece of the full width (no log2w)."""
    import torch

    from vortex_amd import device as vdev

    K = log2_width
    counts = sw.count_batches("node", K)
    rows_h, _, roots = sw.node_rows(K, [K] * max(counts), seed=sw.SEED + 1)
    leaves = torch.from_numpy(rows_h).to(gpu)
    for n in counts:
        exp_h, ok = sw.one_bit_off(roots[:n])
        exp = torch.from_numpy(exp_h).to(gpu)
        out_r, out_m = run.full(torch, gpu, (n + 1, 32)), run.full(torch, gpu, (n + 1,))
        vdev.merkle_nodes(leaves, n, K, expected=exp, roots=out_r, matched=out_m)
        torch.cuda.synchronize()
        w = f"merkle_nodes, log2_width {K}, {n} pieces"
        run.rows(out_r, roots[:n], w, lambda i: f"piece {i}")
        run.verdicts(out_m, ok, w)
    run.unchanged([(leaves, rows_h)], f"merkle_nodes, log2_width {K}")


# ---------------------------------------------------------------------------
# merkle_piece_kernel's tree phase, and the leaf + node pair on the same bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log2_width", range(sw.PIECE_TILE_LOG2 + 1))
def test_pieces_width_shape(built, gpu, log2_width):
    """Whole pieces (every leaf a real hash), every fifth one byte more than
    half, every eleventh empty (its root the pad hash of its own width)."""
    import torch

    K = log2_width
    p = _batch(K)
    bufs = run.buffers(torch, gpu, p.host, p.flipped)
    run.pieces(torch, gpu, K, p.offs, p.lens, bufs, p.roots, lw=p.lw)
    run.ragged(torch, gpu, K, p.offs, p.lens, bufs, p.leaves, p.roots, lw=p.lw)


@pytest.mark.parametrize("log2_width", range(sw.PIECE_TILE_LOG2 + 1))
def test_pieces_count_batches(built, gpu, log2_width):
    import torch

    K = log2_width
    counts = sw.count_batches("piece", K)
    m = max(counts)
    p = sw.Pieces(K, [K] * m, [sw.piece_len(i, K, full=(i % 4 != 3)) for i in range(m)], seed=sw.SEED + 2)
    bufs = run.buffers(torch, gpu, p.host, None)
    for n in counts:
        run.pieces(torch, gpu, K, p.offs[:n], p.lens[:n], bufs, p.roots[:n], what=f"merkle_pieces, {n} pieces")


@pytest.mark.parametrize("log2_width", sw.WIDE)
def test_pieces_two_launches(built, gpu, log2_width):
    """One piece of every width under a batch of 512 or 1,024 slots, and one
    with a single byte in its second 256-leaf tile.  The work area is the
    test's own (the C entry): the tops of the tiles under each piece's own
    root and a width per piece are written, nothing else."""
    import torch

    from vortex_amd._lib import check, lib

    K = log2_width
    p = _batch(K)
    n, ts = p.n, K - sw.PIECE_TILE_LOG2
    bufs = run.buffers(torch, gpu, p.host, p.flipped)
    run.pieces(torch, gpu, K, p.offs, p.lens, bufs, p.roots, lw=p.lw)
    run.ragged(torch, gpu, K, p.offs, p.lens, bufs, p.leaves, p.roots, lw=p.lw)

    T = n << ts
    tile = 1 << sw.PIECE_TILE_LOG2
    want_work = np.full(T * 32 + n + 64, FILL, dtype=np.uint8)
    for i, w in enumerate(p.lw):
        top = max(w - sw.PIECE_TILE_LOG2, 0)
        for t in range(1 << top):
            first = (i << K) + t * tile
            rows = [p.leaves[first + k].tobytes() for k in range(min(tile, 1 << w))]
            at = ((i << ts) + t) * 32
            want_work[at:at + 32] = np.frombuffer(sw.tree_root(rows), dtype=np.uint8)
        want_work[T * 32 + i] = top
    d_offs, d_lens = run.tables(torch, gpu, p.offs, p.lens)
    d_lw = torch.tensor(p.lw, dtype=torch.uint8, device=gpu)
    exp_h, ok = sw.one_bit_off(p.roots)
    exp = torch.from_numpy(exp_h).to(gpu)
    for label, arr, data in bufs:
        work = run.full(torch, gpu, (len(want_work),))
        out_r, out_m = run.full(torch, gpu, (n + 1, 32)), run.full(torch, gpu, (n + 1,))
        check(lib().vx_merkle_device_pieces(data.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), d_lw.data_ptr(), n,
                                            K, work.data_ptr(), out_r.data_ptr(), exp.data_ptr(), out_m.data_ptr(),
                                            int(torch.cuda.current_stream(gpu).cuda_stream)),
              "vx_merkle_device_pieces")
        torch.cuda.synchronize()
        w = f"vx_merkle_device_pieces, log2_width {K}, {label}"
        run.rows(out_r, p.roots, w, lambda i: f"piece {i} (log2w {p.lw[i]}, {p.lens[i]} bytes)")
        run.verdicts(out_m, ok, w)
        got = work.cpu().numpy()
        bad = np.flatnonzero(got != want_work)
        assert bad.size == 0, (f"{w}: {bad.size} bytes of the work area differ, first at byte {bad[0]} "
                               f"(row {bad[0] // 32} of {T}, then {n} widths, then 64 spare bytes)")


# ---------------------------------------------------------------------------
# merkle_root past the counts of test_gpu_merkle_layers.py
# ---------------------------------------------------------------------------
def test_root_of_three_passes(built, gpu):
    """2^19 + 1 rows at height 0: 20 levels are three passes (9 + 9 + 2), and
    the third pads its input of three rows with the pad hash of height 18."""
    import torch

    from vortex_amd import device as vdev

    n = (1 << 19) + 1
    layer_h = sw.random_bytes(sw.SEED + 19, n * 32).reshape(n, 32)
    blob = layer_h.tobytes()
    # the upper half of the padded tree is one row and pad hashes: the root from the two halves
    left = sw.tree_root([blob[32 * k:32 * k + 32] for k in range(1 << 19)])
    right = blob[32 * (n - 1):]
    for h in range(19):
        right = sw.sha256(right + sw.pad_hash(h))
    want = sw.sha256(left + right)
    layer = torch.from_numpy(layer_h).to(gpu)
    root = vdev.merkle_root(layer, 0)
    torch.cuda.synchronize()
    assert root.cpu().numpy().tobytes() == want
    run.unchanged([(layer, layer_h)], "merkle_root")
