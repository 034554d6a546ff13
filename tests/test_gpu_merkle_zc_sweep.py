"""GPU: merkle_zc_piece_kernel on its own, through vx_tuning_merkle_zc_kernel
over torch HBM buffers (a device-visible address is all the kernel asks for).

Every launch of tests/_merkle_zc_sweep.py (built from the kernel's geometry;
tests/test_merkle_zc_cpu.py asserts which classes the launches reach): every
root and verdict against hashlib and against device.merkle_pieces
(merkle_piece_kernel) on the same bytes.  Every byte outside a piece is 0xA5,
so a lane that hashed past a piece's end gets a wrong root.  One case has its
sources in two allocations more than 4 GiB of address apart.
"""
import functools

import numpy as np
import pytest

import _merkle_zc_sweep as zs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _runs():
    return {r.name: r for r in zs.launches(zs.geometry())}


def _names():
    # (the names do not depend on the geometry; collected without the library)
    return [r.name for r in zs.launches(zs.Geo(256, 64, 256, 2))]


@functools.lru_cache(maxsize=None)
def _reference(name):
    run = _runs()[name]
    buf, offs = zs.place(run)
    return (buf, offs) + zs.model(run, buf, offs)


def zc_kernel(dev, srcs, lens, log2w, K, rows):
    """One vx_tuning_merkle_zc_kernel call; returns (roots bytes per piece, verdicts or None)."""
    import torch

    from vortex_amd._lib import tuning
    from vortex_amd.hash_pool import check

    n = len(srcs)
    d_srcs = torch.tensor(np.array(srcs, dtype=np.uint64).view(np.int64), dtype=torch.int64, device=dev)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=dev)
    d_log2w = torch.tensor(log2w, dtype=torch.uint8, device=dev)
    d_roots = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
    d_exp = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev) if rows is not None else None
    d_matched = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) if rows is not None else None
    check(tuning().vx_tuning_merkle_zc_kernel(d_srcs.data_ptr(), d_lens.data_ptr(), d_log2w.data_ptr(), n, K,
                                              d_roots.data_ptr(), d_exp.data_ptr() if rows is not None else None,
                                              d_matched.data_ptr() if rows is not None else None, None),
          "vx_tuning_merkle_zc_kernel", tuning())
    torch.cuda.synchronize()
    raw = d_roots.cpu().numpy().tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(n)], (d_matched.cpu().tolist() if rows is not None else None)


def piece_kernel(d_buf, offs, lens, log2w, K, rows):
    """The same bytes through merkle_piece_kernel (device.merkle_pieces)."""
    import torch

    from vortex_amd import device as vdev

    dev = d_buf.device
    exp = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev).view(-1, 32) if rows is not None else None
    roots, matched = vdev.merkle_pieces(d_buf, torch.tensor(offs, dtype=torch.int64, device=dev),
                                        torch.tensor(lens, dtype=torch.int32, device=dev), K,
                                        log2w=torch.tensor(log2w, dtype=torch.uint8, device=dev), expected=exp)
    torch.cuda.synchronize()
    raw = roots.cpu().numpy().tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(len(offs))], (matched.cpu().tolist() if rows is not None else None)


@pytest.mark.parametrize("name", _names())
def test_launch_matches_hashlib_and_the_piece_kernel(built, gpu, name):
    import torch

    run = _runs()[name]
    buf, offs, roots, rows, verdicts = _reference(name)
    d_buf = torch.from_numpy(buf).to(gpu)
    assert d_buf.data_ptr() % 256 == 0
    lens = [v for v, _ in run.pieces]
    log2w = [lw for _, lw in run.pieces]
    got, matched = zc_kernel(gpu, [d_buf.data_ptr() + o for o in offs], lens, log2w, run.K, rows)
    bad = [i for i in range(len(lens)) if got[i] != roots[i]]
    assert not bad, (name, [(i, run.pieces[i]) for i in bad[:8]])
    assert matched == verdicts
    ref, ref_matched = piece_kernel(d_buf, offs, lens, log2w, run.K, rows)
    assert got == ref and matched == ref_matched
    assert d_buf.cpu().numpy().tobytes() == buf.tobytes()  # the sources are only read


def test_sources_in_two_allocations_more_than_4_gib_apart(built, gpu):
    """Pieces 0, 2, 4 ... in one allocation, 1, 3, 5 ... at the end of a second
    one whose far end lies more than 4 GiB of address from the first: a source
    is a full 64-bit address."""
    import torch

    run = _runs()["lengths"]
    buf, offs, roots, rows, verdicts = _reference("lengths")
    near = torch.from_numpy(buf).to(gpu)
    span = 8 << 30
    other = torch.empty(span + buf.size, dtype=torch.uint8, device=gpu)  # (not filled: only its ends are used)
    # at least one end of an 8 GiB allocation is 4 GiB or more from any address outside it
    at = max((0, span), key=lambda o: abs(other.data_ptr() + o - near.data_ptr()))
    far = other[at:at + buf.size]
    far.copy_(near)
    assert abs(far.data_ptr() - near.data_ptr()) > 4 << 30 and far.data_ptr() % 16 == 0
    srcs = [(near if i % 2 == 0 else far).data_ptr() + o for i, o in enumerate(offs)]
    got, matched = zc_kernel(gpu, srcs, [v for v, _ in run.pieces], [lw for _, lw in run.pieces], run.K, rows)
    assert got == roots and matched == verdicts
    del far, other
    torch.cuda.empty_cache()
