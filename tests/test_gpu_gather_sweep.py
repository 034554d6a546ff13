"""GPU: gather_kernel (vx_gather.hip) on its own, through
vx_tuning_gather_kernel, against a numpy copy.  The engine judges the kernel
by the digests of what it copied, which cannot see a tile written past its
piece's end (arena offsets are aligned, the bytes land in a gap nobody
hashes), a tail or tile copied twice, or a piece copied that the launch does
not gather.  Here the whole arena is compared: the destinations and every byte
outside them, out of an arena filled with 0xA5 from sources that hold no 0xA5.

The shapes are those of tests/_gather_sweep.py, each with max_grid 0 (the
default of 64 workgroups), 1 and 128; tests/test_gather_sweep_cpu.py shows
that they reach every class of tile (words against the block and the unrolled
trip, tail bytes), of piece (tile counts, empty and skipped pieces first, last
and in runs), of table length and of tile count against the grid cap.
"""
import numpy as np
import pytest

import _gather_sweep as gs

pytestmark = pytest.mark.gpu


def _stream(torch, gpu):
    return int(torch.cuda.current_stream(gpu).cuda_stream)


def _launch(torch, gpu, lay, src_base, max_grid, arena=None):
    """One launch through the hook on an arena of 0xA5; returns the arena's
    bytes.  The four tables must come back as they went."""
    from vortex_amd._lib import check, tuning

    tabs = lay.tables(src_base)
    d_src, d_dst, d_lens, d_tfirst = (torch.from_numpy(t.view(np.int64) if t.dtype == np.uint64 else t.view(np.int32))
                                      .to(gpu) for t in tabs)
    if arena is None:
        arena = torch.full((lay.arena_bytes,), gs.FILL, dtype=torch.uint8, device=gpu)
    assert arena.data_ptr() % 16 == 0
    check(tuning().vx_tuning_gather_kernel(d_src.data_ptr(), d_dst.data_ptr(), d_lens.data_ptr(), d_tfirst.data_ptr(),
                                           lay.n, lay.ntiles, arena.data_ptr(), max_grid, _stream(torch, gpu)),
          "vx_tuning_gather_kernel", tuning())
    torch.cuda.synchronize()
    for name, d, t in zip(("src", "dst_off", "lens", "tfirst"), (d_src, d_dst, d_lens, d_tfirst), tabs):
        assert d.cpu().numpy().tobytes() == t.tobytes(), f"{lay.name}: the {name} table was written"
    return arena.cpu().numpy()


def _check(lay, got, max_grid):
    want = gs.model(lay)
    if not np.array_equal(got, want):  # one comparison; the message is worked out only when it fails
        raise AssertionError(f"max_grid {max_grid}: " + gs.first_difference(lay, got, want))


@pytest.mark.parametrize("max_grid", gs.MAX_GRIDS)
@pytest.mark.parametrize("name", list(gs.SHAPES))
def test_gather_equals_a_numpy_copy(built, gpu, name, max_grid):
    import torch

    lay = gs.layout(name)
    source = torch.from_numpy(lay.data).to(gpu)
    assert source.data_ptr() % 16 == 0
    got = _launch(torch, gpu, lay, source.data_ptr(), max_grid)
    _check(lay, got, max_grid)
    assert source.cpu().numpy().tobytes() == lay.data.tobytes(), "the source was written"


def test_gather_from_pinned_host_memory(built, gpu):
    """The sources in a pinned host tensor, read through its device mapping as
    the engine reads a registered buffer; the last source ends on the tensor's
    last byte.  The mapping's address comes from the HIP runtime the library
    is bound to (hipHostGetDevicePointer through ctypes)."""
    import ctypes

    import torch

    from vortex_amd._lib import tuning

    lay = gs.layout("cover")
    host = torch.from_numpy(lay.data).pin_memory()
    assert host.is_pinned()
    fn = tuning().hipHostGetDevicePointer
    fn.argtypes, fn.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_uint], ctypes.c_int
    mapped = ctypes.c_void_p()
    assert fn(ctypes.byref(mapped), ctypes.c_void_p(host.data_ptr()), 0) == 0 and mapped.value
    assert mapped.value % 16 == 0
    for max_grid in (0, 128):
        _check(lay, _launch(torch, gpu, lay, mapped.value, max_grid), max_grid)
    assert host.numpy().tobytes() == lay.data.tobytes(), "the source was written"


def test_gather_writes_over_what_the_arena_held(built, gpu):
    """A second launch into the arena of the first, the other way round in the
    table: every destination holds the second launch's bytes, nothing else
    moved (a tile skipped by the second launch would keep the first's)."""
    import torch

    lay = gs.layout("n9")
    source = torch.from_numpy(lay.data).to(gpu)
    flipped = torch.from_numpy(lay.data ^ 0xFF).to(gpu)  # (differs from the first launch's in every byte)
    arena = torch.full((lay.arena_bytes,), gs.FILL, dtype=torch.uint8, device=gpu)
    _check(lay, _launch(torch, gpu, lay, source.data_ptr(), 0, arena), 0)
    got = _launch(torch, gpu, lay, flipped.data_ptr(), 1, arena)
    want = gs.model(lay)
    inside = want != gs.FILL
    want[inside] ^= 0xFF
    assert np.array_equal(got, want), gs.first_difference(lay, got, want)


def test_gather_entry_checks_its_arguments(built, gpu):
    import torch

    from vortex_amd._lib import VX_EINVAL, tuning

    T = tuning()
    fn = T.vx_tuning_gather_kernel
    lay = gs.layout("n3")
    source = torch.from_numpy(lay.data).to(gpu)
    tabs = lay.tables(source.data_ptr())
    d = [torch.from_numpy(t.view(np.int64) if t.dtype == np.uint64 else t.view(np.int32)).to(gpu) for t in tabs]
    arena = torch.full((lay.arena_bytes,), gs.FILL, dtype=torch.uint8, device=gpu)
    s = _stream(torch, gpu)
    good = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), lay.n, lay.ntiles, arena.data_ptr(), 0, s]
    for k in (0, 1, 2, 3, 6):
        a = list(good)
        a[k] = None
        assert fn(*a) == VX_EINVAL and b"NULL" in T.vx_last_error(), k
    for k, by in ((6, 8), (6, 1), (0, 4), (1, 4), (2, 2), (3, 2)):
        a = list(good)
        a[k] += by
        assert fn(*a) == VX_EINVAL and b"aligned" in T.vx_last_error(), k
    assert fn(None, None, None, None, 0, 0, None, 0, s) == 0  # n == 0 launches nothing
    a = list(good)
    a[5] = 0
    assert fn(*a) == 0  # ntiles == 0 launches nothing
    torch.cuda.synchronize()
    assert (arena.cpu().numpy() == gs.FILL).all(), "a refused or empty call wrote to the arena"
    assert fn(*good) == 0
    torch.cuda.synchronize()
    _check(lay, arena.cpu().numpy(), 0)
