"""GPU: the two kernels that hash zeros from nothing, on their own:
sha1_zero_kernel through device.sha1_zeros / vx_sha1_device_zeros, and
merkle_zero_leaf_kernel through device.merkle_zero_leaves and, with its row
table and full row, through vx_tuning_zero_leaf_kernel.  They judge data the
engine never reads, so nothing downstream would notice a wrong digest.

Everything is bit-exact against hashlib (tests/_zero_sweep.py computes each
length's digest once).  The shapes are those of tests/_zero_sweep.py, and
tests/test_zero_sweep_cpu.py shows that they reach every class of lane the
kernels tell apart: every rem = len & 63 (so every rem & 3; rem & 3 == 2 had
never run on a GPU) at zero, one and more zero blocks, as the wave's longest
lane and below it, and for the leaf kernel stored-as-is lanes in waves of all
three kinds.  Outputs are prefilled and have rows no lane names; those rows are
compared too.

Out of scope: lengths of 2^29 bytes and more, where the bit length's high word
is not zero.  That takes 2^23 serial blocks in one lane (about 6 s), and this
kernel takes no incoming state, so the short cut of test_zero_tail_long_totals
(tests/test_gpu_hybrid_tail_sweep.py) does not apply.
"""
import ctypes
import time

import numpy as np
import pytest

import _zero_sweep as zs

pytestmark = pytest.mark.gpu


def _rows(want):
    return np.frombuffer(b"".join(want), dtype=np.uint8).reshape(len(want), -1)


def _check_digests(what, got, lens, want, rows=None):
    """got[rows[j]] (rows None: got[j]) is lane j's digest want[j]."""
    lens = np.asarray(lens, dtype=np.int64)
    at = np.arange(len(lens)) if rows is None else np.asarray(rows)
    bad = np.flatnonzero((got[at] != _rows(want)).any(axis=1))
    if bad.size:
        j, rem = bad[0], lens[bad] & 63
        raise AssertionError(
            f"{what}: {bad.size} of {len(lens)} digests differ from hashlib, first: lane {j} (row {at[j]}, len "
            f"{lens[j]}, rem {lens[j] & 63}, rem & 3 = {lens[j] & 3}); rem & 3 of all: {sorted(set((rem & 3).tolist()))}; "
            f"lanes: {bad[:16].tolist()}")


def _stream(torch, gpu):
    return int(torch.cuda.current_stream(gpu).cuda_stream)


# ---------------------------------------------------------------------------
# sha1_zero_kernel
# ---------------------------------------------------------------------------
SHA1_LISTS = {"grid": zs.SHA1_GRID, "shuffled": zs.SHA1_SHUFFLED, "long": zs.SHA1_LONG}


@pytest.mark.parametrize("tensor", [False, True], ids=["host-list", "device-tensor"])
@pytest.mark.parametrize("name", list(SHA1_LISTS))
def test_sha1_zeros(built, gpu, name, tensor):
    import torch

    from vortex_amd import device as vdev

    lens = SHA1_LISTS[name]
    arg = torch.tensor(lens, dtype=torch.int32, device=gpu) if tensor else lens
    got = vdev.sha1_zeros(arg).cpu().numpy()
    assert got.shape == (len(lens), 20)
    _check_digests(f"sha1_zeros, {name}", got, lens, [zs.sha1_of_zeros(L) for L in lens])
    if tensor:
        assert arg.cpu().tolist() == lens


@pytest.mark.parametrize("name", list(SHA1_LISTS))
def test_sha1_zeros_raw_writes_its_rows_only(built, gpu, name):
    """vx_sha1_device_zeros itself: the output has a spare row, prefilled; the
    lengths are read only."""
    import torch

    from vortex_amd._lib import check, lib

    lens = SHA1_LISTS[name]
    n = len(lens)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out = torch.full((n + 1, 20), 0xA5, dtype=torch.uint8, device=gpu)
    check(lib().vx_sha1_device_zeros(d_lens.data_ptr(), n, out.data_ptr(), _stream(torch, gpu)), "vx_sha1_device_zeros")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _check_digests(f"vx_sha1_device_zeros, {name}", got, lens, [zs.sha1_of_zeros(L) for L in lens])
    assert (got[n] == 0xA5).all(), "the spare digest row was written"
    assert d_lens.cpu().tolist() == lens, "the lengths were written"


def test_sha1_zeros_one_lane_of_65536_blocks(built, gpu):
    """A 4 MiB lane among short ones: their finished state sits under the
    select for 65,536 iterations.  Measured on an MI355X: 47.4 ms for the call
    and its copy back, 0.724 us per zero block, the zero-tail kernel's figure
    (DESIGN.md §3.8).  Should that ever grow to seconds, shorten the lane."""
    import torch

    from vortex_amd import device as vdev

    lens = zs.SHA1_HUGE
    vdev.sha1_zeros([0, 64])  # (the first launch loads the code object)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = vdev.sha1_zeros(lens).cpu().numpy()
    dt = time.perf_counter() - t0
    print(f"sha1_zeros over {lens}: {dt * 1e3:.1f} ms, {dt * 1e6 / (max(lens) >> 6):.3f} us per block")
    _check_digests("sha1_zeros, 4 MiB lane", got, lens, [zs.sha1_of_zeros(L) for L in lens])


# ---------------------------------------------------------------------------
# merkle_zero_leaf_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tensor", [False, True], ids=["host-list", "device-tensor"])
@pytest.mark.parametrize("name", ["grid", "shuffled"])
def test_merkle_zero_leaves(built, gpu, name, tensor):
    import torch

    from vortex_amd import device as vdev

    lens = {"grid": zs.LEAF_GRID, "shuffled": zs.LEAF_SHUFFLED}[name]
    arg = torch.tensor(lens, dtype=torch.int32, device=gpu) if tensor else lens
    got = vdev.merkle_zero_leaves(arg).cpu().numpy()
    assert got.shape == (len(lens), 32)
    _check_digests(f"merkle_zero_leaves, {name}", got, lens, zs.leaf_want(lens, None))


def _zero_leaf_kernel(torch, gpu, lens, rows_form, full_form):
    """vx_tuning_zero_leaf_kernel over one launch; checks every row of the
    output, the rows no lane names included."""
    from vortex_amd._lib import check, tuning

    n = len(lens)
    rows, out_rows = zs.rows_table(rows_form, n)
    full = zs.full_row(full_form)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=gpu)
    d_rows = torch.tensor(rows, dtype=torch.int32, device=gpu) if rows is not None else None
    out = torch.full((out_rows + 1, 32), 0xFF, dtype=torch.uint8, device=gpu)
    check(tuning().vx_tuning_zero_leaf_kernel(d_rows.data_ptr() if rows is not None else None, d_lens.data_ptr(), n,
                                              out.data_ptr(), full, _stream(torch, gpu)),
          "vx_tuning_zero_leaf_kernel", tuning())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    what = f"zero leaf kernel, n {n}, rows {rows_form}, full row {full_form}"
    _check_digests(what, got, lens, zs.leaf_want(lens, full), rows)
    unnamed = np.setdiff1d(np.arange(out_rows + 1), np.arange(n) if rows is None else np.asarray(rows))
    assert unnamed.size == out_rows + 1 - n
    touched = unnamed[(got[unnamed] != 0xFF).any(axis=1)]
    assert touched.size == 0, f"{what}: rows no lane names were written: {touched[:16].tolist()}"
    assert d_lens.cpu().tolist() == list(lens) and (rows is None or d_rows.cpu().tolist() == rows)


@pytest.mark.parametrize("full_form", zs.FULL_FORMS)
@pytest.mark.parametrize("rows_form", zs.ROWS_FORMS)
@pytest.mark.parametrize("n", zs.LEAF_NS)
def test_zero_leaf_kernel_tables_and_full_rows(built, gpu, n, rows_form, full_form):
    """The row table x the full row x n: lanes of 16384 bytes hold the row
    given, whatever it is (0xC3 bytes are no hash), every other lane hashlib's;
    waves of full lanes only, of none, and of 63 with one other lane."""
    import torch

    _zero_leaf_kernel(torch, gpu, zs.leaf_lens(n), rows_form, full_form)


@pytest.mark.parametrize("full_form", zs.FULL_FORMS)
@pytest.mark.parametrize("rows_form", zs.ROWS_FORMS)
def test_zero_leaf_kernel_cover(built, gpu, rows_form, full_form):
    """Every rem of each band of z beside full lanes: the wave's longest lanes
    with a full row given, below the full lanes' 256 blocks without."""
    import torch

    _zero_leaf_kernel(torch, gpu, zs.LEAF_COVER, rows_form, full_form)


def test_zero_leaf_entry_checks_its_arguments(built, gpu):
    import torch

    from vortex_amd._lib import VX_EINVAL, tuning

    T = tuning()
    fn = T.vx_tuning_zero_leaf_kernel
    lens = torch.tensor([1, 16384, 70, 2], dtype=torch.int32, device=gpu)
    rows = torch.tensor([3, 2, 1, 0], dtype=torch.int32, device=gpu)
    out = torch.full((5, 32), 0xFF, dtype=torch.uint8, device=gpu)
    full = ctypes.create_string_buffer(zs.full_row("c3"), 32)
    s = _stream(torch, gpu)
    assert fn(rows.data_ptr(), None, 4, out.data_ptr(), full, s) == VX_EINVAL and b"NULL" in T.vx_last_error()
    assert fn(rows.data_ptr(), lens.data_ptr(), 4, None, full, s) == VX_EINVAL and b"NULL" in T.vx_last_error()
    assert fn(None, None, 4, None, None, s) == VX_EINVAL
    for bad in ((rows.data_ptr(), lens.data_ptr(), out.data_ptr() + 8), (rows.data_ptr(), lens.data_ptr() + 2, out.data_ptr()),
                (rows.data_ptr() + 1, lens.data_ptr(), out.data_ptr())):
        assert fn(bad[0], bad[1], 4, bad[2], full, s) == VX_EINVAL and b"aligned" in T.vx_last_error()
    assert fn(None, None, 0, None, None, s) == 0  # n == 0 launches nothing
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xFF).all(), "a refused call wrote leaf rows"
    assert fn(rows.data_ptr(), lens.data_ptr(), 4, out.data_ptr(), full, s) == 0
    torch.cuda.synchronize()
    _check_digests("after the refused calls", out.cpu().numpy(), [1, 16384, 70, 2],
                   zs.leaf_want([1, 16384, 70, 2], zs.full_row("c3")), [3, 2, 1, 0])


def test_synth_fill_checks_the_tensor_size(built, gpu):
    """device.synth_fill refuses a batch that ends past its tensor and writes
    nothing."""
    import torch

    from vortex_amd import device as vdev

    data = torch.full((4 * 256,), 0xEE, dtype=torch.uint8, device=gpu)
    for n, plen, stride in ((5, 256, None), (4, 257, None), (4, 200, 300), (1, 1025, None)):
        with pytest.raises(ValueError, match="exceeds"):
            vdev.synth_fill(data, n, plen, stride=stride)
    torch.cuda.synchronize()
    assert bool((data == 0xEE).all()), "a refused fill wrote bytes"
    vdev.synth_fill(data, 4, 200, stride=256)  # the last piece may end before the tensor does
    vdev.synth_fill(data, 0, 4096)
    torch.cuda.synchronize()
    got = data.cpu().numpy().reshape(4, 256)
    assert (got[:, 200:] == 0xEE).all() and not (got[:, :200] == 0xEE).all()
