"""GPU: the resumable chunk kernel (sha1_ragged_split_kernel<true>, launch_chunk)
on its own, through vx_tuning_chunk_kernel, at the edges of its own loops.

The kernel carries a chaining state across launches, and hashlib cannot start
from one, so the yardstick is the state-level model of tests/_sha1_model.py
(pinned to hashlib by tests/test_sha1_model_cpu.py); where a lane starts its
piece (poff == 0) or a chain ends, hashlib is compared as well.  The shapes
are tests/_sha1_sweep.py's chunk recipes; tests/test_sha1_sweep_cpu.py shows
that they take every class of class_chunk.  Everything is bit-exact.  Rules,
as in test_gpu_sha1_sweep.py:

  * one random host array per batch, the chunks at 16-byte aligned offsets
    inside it, so the bytes around every chunk are random, never zero;
  * the state and digest tables are prefilled with 0xA5 and have spare rows,
    `pids` is a random permutation into them: rows no lane names stay 0xA5;
  * the incoming state of a resumed lane is random words, not a real prefix,
    and a lane with poff == 0 gets a random row that it must ignore;
  * every state row is compared, not only the digests: a lane that does not
    end its piece must store the model's state and leave its digest row
    alone, a lane that ends it must leave its state row alone.

What the re-verify and hybrid paths never form, and this file does: whole-block
lanes of every nfull % kBlockRing (5 among them), waves of one final lane
among whole-block lanes and the reverse, waves with no phase 2 after one and
more trips of phase 1, and resumed final chunks of pieces of 512 MiB and more
(both forms of the padding: the phase 2 select and padw[14..15]).

A disagreement between the producer's and the consumer's barrier counts would
show as a hang, not as a wrong digest: if this file hangs, read the code.
"""
import hashlib

import numpy as np
import pytest

import _sha1_model as md
import _sha1_sweep as sw

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5
_cache = {}


def _dev(torch, gpu, a, dtype):
    """A host array of unsigned words as a device tensor of the signed type of
    the same width (the kernel reads the bits)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.itemsize])).to(gpu)


def _launch(torch, gpu, data, offs, lens, pids, poffs, tlens, d_states, d_dig):
    """One launch over device tables; returns (states, digests) as host arrays."""
    from vortex_amd._lib import check, tuning

    t = [_dev(torch, gpu, offs, np.uint64), _dev(torch, gpu, lens, np.uint32), _dev(torch, gpu, pids, np.uint32),
         _dev(torch, gpu, poffs, np.uint64), _dev(torch, gpu, tlens, np.uint64)]
    check(tuning().vx_tuning_chunk_kernel(data.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), len(lens),
                                          t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), d_states.data_ptr(),
                                          d_dig.data_ptr(), int(torch.cuda.current_stream(gpu).cuda_stream)),
          "vx_tuning_chunk_kernel", tuning())
    torch.cuda.synchronize()
    return d_states.cpu().numpy().view(np.uint32), d_dig.cpu().numpy()


def _tables(torch, gpu, rows, pids, states_in):
    """(host state table, device state table, device digest table): 0xA5
    everywhere, the lanes' incoming rows at pids."""
    table = np.full((rows, 5), FILL32, dtype=np.uint32)
    table[pids] = states_in
    return table, _dev(torch, gpu, table, np.uint32), torch.full((rows, 20), 0xA5, dtype=torch.uint8, device=gpu)


def _model(host, offs, lens, final, poffs, tlens, states_in):
    """(state after the lane's whole blocks [n, 5], digest rows of the final
    lanes): the model from each lane's incoming state, the initial value where
    poff == 0."""
    resumed = np.array([p > 0 for p in poffs])
    s = md.run_blocks(np.where(resumed[:, None], states_in, md.IV), host, offs, lens)
    fin = np.flatnonzero(final)
    rem = lens[fin] & 63
    tail = md.tail_rows(host, offs[fin] + (lens[fin] & ~63), rem)
    return s, md.digest_rows(md.finish(s[fin], tail, rem, [tlens[i] for i in fin]))


def _check(what, got_states, got_dig, table, pids, final, want_states, want_dig):
    """Every row of both tables after a launch."""
    fin, rest = np.flatnonzero(final), np.flatnonzero(~final)
    bad = rest[(got_states[pids[rest]] != want_states[rest]).any(axis=1)]
    assert bad.size == 0, f"{what}: {bad.size} stored states differ from the model, first: lane {bad[0]}"
    assert (got_dig[pids[rest]] == 0xA5).all(), f"{what}: a lane that does not end its piece wrote a digest row"
    bad = fin[(got_dig[pids[fin]] != want_dig).any(axis=1)]
    assert bad.size == 0, f"{what}: {bad.size} digests differ from the model, first: lane {bad[0]}"
    assert (got_states[pids[fin]] == table[pids[fin]]).all(), f"{what}: a lane that ends its piece wrote its state row"
    spare = np.setdiff1d(np.arange(len(table)), pids)
    assert spare.size and (got_states[spare] == FILL32).all() and (got_dig[spare] == 0xA5).all(), \
        f"{what}: a spare row was written"


# ---------------------------------------------------------------------------
# 1. The recipes, one launch each
# ---------------------------------------------------------------------------
def _recipe(name):
    """Everything a recipe's launch needs and must give, built once."""
    if name not in _cache:
        lanes = sw.chunk_batch(name)
        n = len(lanes)
        assert n % sw.WAVE == 1
        lens = np.array([x[0] for x in lanes], dtype=np.int64)
        final = np.array([x[1] for x in lanes])
        offs, size = sw.layout(lens.tolist(), gap=16)
        offs = np.array(offs, dtype=np.int64)
        rng = np.random.default_rng(n + len(name))
        host = rng.integers(0, 256, size + 64, dtype=np.uint8)
        i = np.arange(n)
        # 'final': every lane resumes; the others: every fourth lane starts its piece
        poffs = 64 * (1 + i % 5) if name == "final" else 64 * (i % 4)
        tlens = np.where(final, poffs + lens, poffs + lens + 64 * (1 + i % 3) + i % 64)
        rows = n + 7
        pids = rng.permutation(rows)[:n]
        states_in = rng.integers(0, 2 ** 32, (n, 5), dtype=np.uint32)
        want_states, want_dig = _model(host, offs, lens, final, poffs.tolist(), tlens.tolist(), states_in)
        _cache[name] = dict(host=host, offs=offs, lens=lens, final=final, poffs=poffs, tlens=tlens, rows=rows,
                            pids=pids, states_in=states_in, want_states=want_states, want_dig=want_dig)
    return _cache[name]


def _run_recipe(torch, gpu, r, host, what, count=None):
    n = count or len(r["lens"])
    table, d_states, d_dig = _tables(torch, gpu, r["rows"], r["pids"][:n], r["states_in"][:n])
    got = _launch(torch, gpu, torch.from_numpy(host).to(gpu), r["offs"][:n], r["lens"][:n], r["pids"][:n],
                  r["poffs"][:n], r["tlens"][:n], d_states, d_dig)
    fin = np.flatnonzero(r["final"][:n])
    _check(what, *got, table, r["pids"][:n], r["final"][:n], r["want_states"][:n], r["want_dig"][:len(fin)])
    return got


@pytest.mark.parametrize("name", sw.CHUNK_RECIPES)
def test_chunk_recipes(built, gpu, name):
    import torch

    r = _recipe(name)
    _, got_dig = _run_recipe(torch, gpu, r, r["host"], name)
    # where a final lane is its whole piece, hashlib says the same
    whole = np.flatnonzero(r["final"] & (r["poffs"] == 0))
    assert (name == "final") == (whole.size == 0)
    view = memoryview(r["host"])
    for k in whole:
        o, ln = int(r["offs"][k]), int(r["lens"][k])
        assert got_dig[r["pids"][k]].tobytes() == hashlib.sha1(view[o:o + ln]).digest(), (name, k, ln)


# ---------------------------------------------------------------------------
# 2. Chains: pieces cut at the ring's edges, one launch per round
# ---------------------------------------------------------------------------
def test_chunk_chains(built, gpu):
    """After every launch the whole state table is the model's (a piece that
    has ended keeps the state its last whole-block chunk left), and a piece's
    digest row is 0xA5 until its last chunk and hashlib's after it."""
    import torch

    plan = sw.chain_plan()
    n = len(plan)
    lens = np.array([L for L, _ in plan], dtype=np.int64)
    offs, size = sw.layout(lens.tolist(), gap=16)
    offs = np.array(offs, dtype=np.int64)
    rng = np.random.default_rng(n)
    host = rng.integers(0, 256, size + 64, dtype=np.uint8)
    view = memoryview(host)
    want_dig = np.frombuffer(b"".join(hashlib.sha1(view[o:o + L]).digest()
                                      for o, L in zip(offs.tolist(), lens.tolist())), dtype=np.uint8).reshape(n, 20)
    rows = n + 5
    pids = rng.permutation(rows)[:n]
    table = np.full((rows, 5), FILL32, dtype=np.uint32)
    d_states = _dev(torch, gpu, table.copy(), np.uint32)
    d_dig = torch.full((rows, 20), 0xA5, dtype=torch.uint8, device=gpu)
    data = torch.from_numpy(host).to(gpu)
    exp_dig = np.full((rows, 20), 0xA5, dtype=np.uint8)
    done = np.zeros(n, dtype=np.int64)  # bytes of each piece hashed so far
    for rnd in range(max(len(c) for _, c in plan)):
        live = rng.permutation([k for k, (_, c) in enumerate(plan) if len(c) > rnd])
        clen = np.array([plan[k][1][rnd] for k in live], dtype=np.int64)
        final = np.array([len(plan[k][1]) == rnd + 1 for k in live])
        assert final.any() == (rnd > 0)
        # the model goes on from its own table: IV where the piece starts (what the device row holds is ignored)
        start = np.where((done[live] > 0)[:, None], table[pids[live]], md.IV)
        s = md.run_blocks(start, host, offs[live] + done[live], clen)
        got_states, got_dig = _launch(torch, gpu, data, offs[live] + done[live], clen, pids[live], done[live],
                                      lens[live], d_states, d_dig)
        table[pids[live[~final]]] = s[~final]
        exp_dig[pids[live[final]]] = want_dig[live[final]]
        done[live] += clen
        assert (got_states == table).all(), f"round {rnd}: {(got_states != table).any(axis=1).sum()} state rows differ"
        bad = np.flatnonzero((got_dig != exp_dig).any(axis=1))
        assert bad.size == 0, f"round {rnd}: {bad.size} digest rows differ from hashlib / 0xA5"
    assert (done == lens).all() and (exp_dig[pids] == want_dig).all()


# ---------------------------------------------------------------------------
# 3. Totals of 512 MiB and more, on resumed final chunks
# ---------------------------------------------------------------------------
def test_chunk_long_totals(built, gpu):
    """bits_hi per lane: each wave mixes totals of 2^29, 2^32 + 64 and 2^35
    bytes with short ones; one padding block (padw[14..15]) and two (the
    phase 2 select at k >= 14).  n % 64 == 63."""
    import torch

    b = sw.chunk_long_batch()
    n = len(b.lens)
    assert n % sw.WAVE == 63
    final = np.ones(n, dtype=bool)
    rows = n + 3
    pids = np.random.default_rng(n).permutation(rows)[:n]
    table, d_states, d_dig = _tables(torch, gpu, rows, pids, b.states)
    want_states, want_dig = _model(b.buf, b.offs, b.lens, final, b.poffs, b.tlens, b.states)
    got = _launch(torch, gpu, torch.from_numpy(b.buf).to(gpu), b.offs, b.lens, pids, b.poffs, b.tlens, d_states, d_dig)
    _check("long totals", *got, table, pids, final, want_states, want_dig)
    view = memoryview(b.buf)
    whole = [k for k in range(n) if b.poffs[k] == 0]
    assert whole
    for k in whole:
        o, ln = int(b.offs[k]), int(b.lens[k])
        assert got[1][pids[k]].tobytes() == hashlib.sha1(view[o:o + ln]).digest()


# ---------------------------------------------------------------------------
# 4. Bytes outside the chunks do not matter;  5. a last wave of 63 lanes
# ---------------------------------------------------------------------------
def test_chunk_outside_bytes_do_not_matter(built, gpu):
    import torch

    from test_gpu_sha1_sweep import _outside_flipped

    r = _recipe("one final")
    a = _run_recipe(torch, gpu, r, r["host"], "as laid out")
    b = _run_recipe(torch, gpu, r, _outside_flipped(r["host"], r["offs"].tolist(), r["lens"].tolist()),
                    "outside bytes inverted")
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_chunk_partial_last_wave(built, gpu):
    """n % 64 == 63 (every recipe's launch has n % 64 == 1): the first lanes of
    a recipe up to a wave of two kinds of lane, cut one lane short."""
    import torch

    r = _recipe("one whole")
    lanes = sw.chunk_batch("one whole")
    w = next(k for k in range(2, len(lanes) // sw.WAVE) if len(set(lanes[sw.WAVE * k:sw.WAVE * k + 63])) == 2)
    n = sw.WAVE * w + 63
    _run_recipe(torch, gpu, r, r["host"], f"the first {n} lanes", count=n)
