"""GPU: sha1_zero_run_kernel on its own (vx_tuning_zero_run_kernel; DESIGN.md
§3.8, §6.11): the kernel that takes a hybrid piece's SHA-1 state across a chunk
the file system never wrote.

It starts from a chaining state and leaves one, so the yardstick is the
state-level model of tests/_sha1_model.py (zero_blocks), bit-exact; two
compositions end in a digest and are held to zero_tail and to hashlib.  Rules:

  * the state table is random words for the lanes that continue a piece, 0xA5
    for every other row, and has a spare row; rows no lane names, and the
    spare, are compared too;
  * a lane with poff == 0 starts from the initial value over a garbage row;
  * pids are a sparse permutation: lane j's row is not row j.
"""
import hashlib

import numpy as np
import pytest

import _sha1_model as md

pytestmark = pytest.mark.gpu

BLOCKS = (1, 2, 63, 64, 65, 4096)
_cache = {}


def _dev(torch, gpu, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize])).to(gpu)


def _launch(torch, gpu, pids, poffs, blocks, d_states):
    from vortex_amd._lib import check, tuning

    t = [_dev(torch, gpu, a, np.uint32) for a in (pids, poffs, blocks)]
    check(tuning().vx_tuning_zero_run_kernel(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(pids),
                                             d_states.data_ptr(), int(torch.cuda.current_stream(gpu).cuda_stream)),
          "vx_tuning_zero_run_kernel", tuning())
    torch.cuda.synchronize()
    return d_states.cpu().numpy().view(np.uint32)


NS = (1, 63, 64, 65, 130)
KINDS = {  # block counts per lane: every count mixed within a wave, and one count per wave
    "mixed": lambda n, j: BLOCKS[j % len(BLOCKS)],
    "uniform": lambda n, j: BLOCKS[(j // 64 + n) % len(BLOCKS)],
}


def _inputs(n, blocks_of, seed):
    """(pids, poffs, blocks, table before): n lanes over a table of 3 n + 1 rows and a spare."""
    rng = np.random.default_rng(seed)
    rows = 3 * n + 2
    pids = rng.permutation(rows - 1)[:n].astype(np.uint32)
    blocks = np.array([blocks_of(j) for j in range(n)], dtype=np.uint32)
    poffs = np.where(np.arange(n) % 3 == 1, 0, 64 * rng.integers(1, 1 << 20, n)).astype(np.uint32)
    before = np.full((rows, 5), 0xA5A5A5A5, dtype=np.uint32)
    before[pids] = rng.integers(0, 1 << 32, (n, 5), dtype=np.uint64).astype(np.uint32)  # garbage where poff == 0
    return pids, poffs, blocks, before


def _after(cases):
    """The tables after the launch, by the model: one zero_blocks call over
    every lane of every case (the model's time goes with the longest run, not
    with the lanes)."""
    start = np.concatenate([np.where((poffs == 0)[:, None], md.IV, before[pids]) for pids, poffs, _, before in cases])
    end = md.zero_blocks(start, np.concatenate([c[2] for c in cases]))
    out, at = [], 0
    for pids, _, _, before in cases:
        after = before.copy()
        after[pids] = end[at:at + len(pids)]
        at += len(pids)
        out.append(after)
    return out


def _grid():
    """Every (kind, n) case with its expected table; the model runs once."""
    if "grid" not in _cache:
        keys = [(kind, n) for kind in KINDS for n in NS]
        cases = [_inputs(n, lambda j: KINDS[kind](n, j), 1000 * k + n) for k, (kind, n) in enumerate(keys)]
        _cache["grid"] = {key: c + (a,) for key, c, a in zip(keys, cases, _after(cases))}
    return _cache["grid"]


def _check(what, got, want, pids):
    bad = np.flatnonzero((got[pids] != want[pids]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} state rows differ from the model, first: lane {bad[0]}"
    rest = np.setdiff1d(np.arange(len(want)), pids)
    assert (got[rest] == want[rest]).all(), f"{what}: a row no lane names, or the spare row, was written"


@pytest.mark.parametrize("n", NS)
def test_mixed_and_uniform_block_counts(built, gpu, n):
    """Every block count mixed within a wave (the loop runs to the wave's
    largest and the others hold under a select), then one count per wave."""
    import torch

    for kind in KINDS:
        pids, poffs, blocks, before, after = _grid()[kind, n]
        assert (poffs == 0).any() or n == 1
        got = _launch(torch, gpu, pids, poffs, blocks, _dev(torch, gpu, before, np.uint32))
        _check(f"{kind}, n = {n}", got.reshape(-1, 5), after, pids)


def test_first_lane_from_the_initial_value(built, gpu):
    """n == 1 with poff == 0 (the n == 1 case above continues a state)."""
    import torch

    before = np.full((3, 5), 0xA5A5A5A5, dtype=np.uint32)
    before[1] = [1, 2, 3, 4, 5]
    after = before.copy()
    after[1] = md.zero_blocks(md.iv(1), [65])[0]
    got = _launch(torch, gpu, [1], [0], [65], _dev(torch, gpu, before, np.uint32))
    _check("one lane", got.reshape(-1, 5), after, np.array([1]))


def test_chain_of_three_launches(built, gpu):
    """A piece with three hole chunks in a row: each launch continues the
    last one's rows; checked after each."""
    import torch

    n = 70
    case = _inputs(n, lambda j: BLOCKS[j % 5], 77)
    pids, poffs, blocks, before = case
    want = _after([case])[0]
    d = _dev(torch, gpu, before, np.uint32)
    for k in range(3):
        if k:
            poffs = poffs + 64 * blocks  # past the start now: the row is read
            want = want.copy()
            want[pids] = md.zero_blocks(want[pids], blocks)
        got = _launch(torch, gpu, pids, poffs, blocks, d)
        _check(f"launch {k}", got.reshape(-1, 5), want, pids)


def test_zero_run_then_zero_tail(built, gpu):
    """Zeros taken in two steps are zeros: a run of z blocks, then the tail
    kernel over a piece that is pl - 64 z' bytes of pad behind them, equals the
    model's zero_tail over the summed zeros."""
    import torch

    from vortex_amd._lib import check, tuning

    n, pl = 66, 1 << 16
    rng = np.random.default_rng(5)
    runs = rng.integers(1, 200, n).astype(np.uint32)
    lens = 64 * rng.integers(1, 300, n).astype(np.uint32)      # the data in front of the run (whole blocks)
    states = rng.integers(0, 1 << 32, (n, 5), dtype=np.uint64).astype(np.uint32)
    d_states = _dev(torch, gpu, states, np.uint32)
    _launch(torch, gpu, np.arange(n), lens, runs, d_states)
    tlen = lens + 64 * runs
    pads = (pl - tlen).astype(np.uint32)
    assert (pads > 0).all()
    t = [_dev(torch, gpu, a, dt) for a, dt in ((np.zeros(64), np.uint8), (np.zeros(n), np.uint64), (tlen, np.uint32),
                                               (pads, np.uint32))]
    dig = torch.full((n + 1, 20), 0xA5, dtype=torch.uint8, device=gpu)
    check(tuning().vx_tuning_zero_tail_kernel(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, pl,
                                              d_states.data_ptr(), dig.data_ptr(),
                                              int(torch.cuda.current_stream(gpu).cuda_stream)),
          "vx_tuning_zero_tail_kernel", tuning())
    torch.cuda.synchronize()
    # the model: one tail over data_len = lens, pad = everything behind it
    want = md.digest_rows(md.zero_tail(states, np.zeros(64, dtype=np.uint8), np.zeros(n), lens, pl - lens))
    got = dig.cpu().numpy()
    assert (got[:n] == want).all() and (got[n] == 0xA5).all()


def test_initial_value_zero_run_then_chunk_kernel(built, gpu):
    """IV -> zero run -> the chunk kernel over real bytes, final: the digest is
    hashlib.sha1(zeros + data)."""
    import torch

    from vortex_amd._lib import check, tuning

    rng = np.random.default_rng(6)
    runs = [1, 5, 64, 4096, 7, 300]
    datas = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in (1, 64, 100, 16384, 55, 4096 + 63)]
    n = len(runs)
    d_states = _dev(torch, gpu, np.full((n + 1, 5), 0xA5A5A5A5), np.uint32)
    _launch(torch, gpu, np.arange(n), np.zeros(n), runs, d_states)
    offs = np.cumsum([0] + [(len(d) + 15) // 16 * 16 for d in datas])
    buf = np.zeros(offs[-1] + 64, dtype=np.uint8)
    for o, d in zip(offs, datas):
        buf[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    poffs = 64 * np.array(runs)
    lens = np.array([len(d) for d in datas])
    t = [_dev(torch, gpu, a, dt) for a, dt in ((buf, np.uint8), (offs[:n], np.uint64), (lens, np.uint32),
                                               (np.arange(n), np.uint32), (poffs, np.uint64), (poffs + lens, np.uint64))]
    dig = torch.full((n + 1, 20), 0xA5, dtype=torch.uint8, device=gpu)
    check(tuning().vx_tuning_chunk_kernel(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, t[3].data_ptr(),
                                          t[4].data_ptr(), t[5].data_ptr(), d_states.data_ptr(), dig.data_ptr(),
                                          int(torch.cuda.current_stream(gpu).cuda_stream)),
          "vx_tuning_chunk_kernel", tuning())
    torch.cuda.synchronize()
    got = dig.cpu().numpy()
    for k in range(n):
        assert got[k].tobytes() == hashlib.sha1(bytes(64 * runs[k]) + datas[k]).digest(), k
    assert (got[n] == 0xA5).all()


def test_entry_checks_its_arguments(built, gpu):
    import torch

    from vortex_amd._lib import VX_EINVAL, tuning

    x = torch.zeros(64, dtype=torch.uint8, device=gpu).data_ptr()
    fn = tuning().vx_tuning_zero_run_kernel
    for k in (0, 1, 2, 4):
        args = [x, x, x, 1, x, None]
        args[k] = None
        assert fn(*args) == VX_EINVAL and b"NULL" in tuning().vx_last_error()
    assert fn(None, None, None, 0, None, None) == 0  # n == 0 launches nothing
