"""CPU: the hybrid re-verify's round planner over file holes
(vortex_amd/csrc/vx_hybrid_rounds.hpp with the scan of vx_extents.hpp as its
hole predicate), run as a stand-alone program
(tests/native/hybrid_holes_dump.cpp) under ASan + UBSan over the sparse torrents
of tests/_hybrid_sparse.py and replayed in Python.

The replay does what the engine does with a round: it stages the reads, runs
the SHA-1 lanes, the zero-run lanes and the tail lanes from one chaining state
per piece, hashes the block table's entries, and must arrive at hashlib's
digests and roots of the files read the ordinary way.  The chaining state is
carried two ways.  ModelChain is tests/_sha1_model.py: run_blocks for lanes,
zero_blocks for zero-run lanes, zero_tail for tails.  The model costs about
1 ms per 64-byte block in sequence, whatever the lanes, and a 1 MiB piece is
16,384 of them, so it replays the main torrent of the 1 MiB layout once (40 s)
and a torrent of 128 KiB pieces in 32 KiB chunks with the same masks and file
ends.  HashlibChain feeds a hashlib object the same bytes (zeros for a zero
run and a tail) and replays every torrent, at every stage size and range.

Counter assertions are skipped where the file system reports no holes; verdict
assertions always hold."""
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _hybrid_sparse as hs
import _sha1_model as md
from _sparse import NO_HOLES, holes_reported
from conftest import ROOT

BLOCK = hs.BLOCK


def _build(tmp, name):
    exe = tmp / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("hhd")
    return _build(tmp, "hybrid_holes_dump"), _build(tmp, "hybrid_rounds_dump")


@pytest.fixture(scope="module")
def torrents(tmp_path_factory):
    d = tmp_path_factory.mktemp("hsparse")
    return {t["name"]: t for t in hs.all_torrents(d)}, holes_reported(d)


def _lines(exe, args, stdin):
    out = subprocess.run([str(exe)] + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.rstrip("\n").split("\n")


def _dump(exe, t, mode, stage, chunk=0, budget=0, first=0, count=-1):
    lines = _lines(exe, [mode, t["pl"], first, count, stage, chunk, budget],
                   "".join(f"{n} {p}\n" for n, p in zip(t["flens"], t["paths"])))
    rounds = []
    for ln in lines[:-1]:
        tag, *v = ln.split()
        v = [int(x) for x in v]
        if tag == "R":
            rounds.append(dict(new=v[0], end=v[1], w_first=v[2], w_n=v[3], K=v[4], data_blocks=v[5], bytes=v[6],
                               file_bytes=v[7], reads=[], lanes=[], tails=[], table=[], hole=[(0, 0)], runs=[],
                               whole=[]))
        else:
            rounds[-1][{"r": "reads", "l": "lanes", "z": "tails", "t": "table", "H": "hole", "h": "runs",
                        "w": "whole"}[tag]].append(tuple(v))
    return rounds, json.loads(lines[-1]), lines[:-1]


class HashlibChain:
    """A piece's chain in a hashlib object: it takes zeros where the kernels
    take none."""

    def __init__(self):
        self.h = {}

    def lanes(self, stage, lanes):
        out = {}
        for at, ln, pid, poff, tlen in lanes:
            assert (pid in self.h) == (poff != 0), "a lane past the piece's start continues a state"
            self.h.setdefault(pid, hashlib.sha1()).update(bytes(stage[at:at + ln]))
            if poff + ln == tlen:
                out[pid] = self.h[pid].digest()
        return out

    def zero_runs(self, runs):
        for pid, poff, blocks in runs:
            assert (pid in self.h) == (poff != 0), "a run that starts the piece starts from the initial value"
            self.h.setdefault(pid, hashlib.sha1()).update(bytes(64 * blocks))

    def tails(self, stage, tails):
        out = {}
        for at, dl, pad, pid in tails:
            assert (pid in self.h) == (dl >> 6 != 0)
            h = self.h.setdefault(pid, hashlib.sha1())
            h.update(bytes(stage[at:at + (dl & 63)]) + bytes(pad))
            out[pid] = h.digest()
        return out

    def flush(self):
        return {}


class ModelChain:
    """A piece's chain as a state row of tests/_sha1_model.py, as the kernels keep it."""

    def __init__(self):
        self.s = {}
        self.held = []  # tail lanes: (pid, state row, the tail's bytes, data_len, pad_len)

    def _rows(self, pids, fresh):
        return np.stack([md.IV if f else self.s[p] for p, f in zip(pids, fresh)]) if pids else md.iv(0)

    def lanes(self, stage, lanes):
        if not lanes:
            return {}
        buf = np.frombuffer(bytes(stage) + bytes(64), dtype=np.uint8)
        at, ln, pid, poff, tlen = (np.array(c, dtype=np.int64) for c in zip(*lanes))
        s = md.run_blocks(self._rows(list(pid), list(poff == 0)), buf, at, ln)
        final = poff + ln == tlen
        rem = ln & 63
        fin = md.finish(s, md.tail_rows(buf, at + (ln & ~63), rem), rem, tlen)
        out = {}
        for k, p in enumerate(pid):
            self.s[int(p)] = s[k]
            if final[k]:
                out[int(p)] = md.digest_rows(fin[k:k + 1])[0].tobytes()
        return out

    def zero_runs(self, runs):
        if not runs:
            return
        pid, poff, blocks = zip(*runs)
        s = md.zero_blocks(self._rows(list(pid), [o == 0 for o in poff]), blocks)
        for k, p in enumerate(pid):
            self.s[p] = s[k]

    def tails(self, stage, tails):
        """Kept for one zero_tail call in flush(): the model's time goes with
        the longest pad, not with the lanes, and nothing reads a tail's result
        before the call ends."""
        for at, dl, pad, pid in tails:
            state = md.IV if dl >> 6 == 0 else self.s[pid]
            self.held.append((pid, state.copy(), bytes(stage[at:at + (dl & 63)]).ljust(64, b"\xff"), dl, pad))
        return {}

    def flush(self):
        if not self.held:
            return {}
        pid, states, tail, dl, pad = zip(*self.held)
        buf = np.frombuffer(b"".join(tail), dtype=np.uint8)
        rows = md.digest_rows(md.zero_tail(np.stack(states), buf, 64 * np.arange(len(pid)), dl, pad))
        return {p: rows[k].tobytes() for k, p in enumerate(pid)}


def _zero_runs(n, msk):
    """Hole chunks of an n-chunk piece (bit j of msk: chunk j unwritten) with a written chunk behind them."""
    return sum(1 for j in range(n) if msk >> j & 1 and (~msk & ((1 << n) - 1)) >> (j + 1))


# of _hybrid_sparse.main_torrent: file 0's sixteen masks, then every mask of every file end
MAIN_ZERO_RUNS = sum(_zero_runs(4, msk) for msk in range(16)) + sum(
    _zero_runs(k + 1, msk) for k in range(4) for msk in range(1 << (k + 1)))


def _root(rows):
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


def replay(exe, t, stage, chain, reported, chunk=0, budget=0, first=0, count=-1):
    """The planner's rounds over torrent t with its files' holes, the kernels
    replaced as said above; returns (rounds, summary, per piece (SHA-1, root))."""
    from vortex_amd import hybrid, sparse

    pl, flens = t["pl"], t["flens"]
    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(flens, pl)
    if count < 0:
        count = len(dlen) - first
    # the model's scan and the planner's before anything reads the files
    model = sparse.hybrid_read_bytes(t["paths"], flens, pl, chunk or None, first, count)
    masks, extents = sparse.hole_chunks(t["paths"], flens, pl, chunk or None)
    rounds, summary, _ = _dump(exe, t, "holes", stage, chunk, budget, first, count)
    real = [open(p, "rb").read().ljust(n, b"\xee")[:n] for p, n in zip(t["paths"], flens)]
    Ck = summary["chunk"]
    assert Ck == sparse.hybrid_chunk(pl, chunk or None)
    budget = summary["row_budget"]
    fed = {}            # pid -> bytes of the piece the chain has taken
    done1, done2, whole = {}, {}, {}
    read_chunks = []    # (piece, chunk) of every chunk read
    leaves, window, next_piece = {}, None, first
    for r in rounds:
        if r["new"]:
            assert window is None and r["w_first"] == next_piece
            window = (r["w_first"], r["w_n"], r["K"])
            assert (r["w_n"] << r["K"]) <= budget, "the row budget holds, whole-hole windows included"
            leaves = {}
        else:
            assert not r["whole"], "whole-hole pieces are named in their window's first round"
        assert window == (r["w_first"], r["w_n"], r["K"])
        w_first, w_n, K = window
        assert r["bytes"] <= stage
        st = bytearray(r["bytes"])
        filled = []
        for f, off, ln, at, piece in r["reads"]:
            assert at % BLOCK == 0 and ln > 0 and off + ln <= flens[f] and at + ln <= r["bytes"]
            assert findex[piece] == f and foff[piece] <= off < foff[piece] + dlen[piece]
            st[at:at + ln] = real[f][off:off + ln]
            filled.append((at, at + ln))
            lo = off
            while lo < off + ln:  # the chunks of the pieces this read covers
                i = next(p for p in range(first, first + count) if findex[p] == f and foff[p] <= lo < foff[p] + dlen[p])
                k = (lo - foff[i]) // Ck
                hi = min(foff[i] + min(dlen[i], (k + 1) * Ck), off + ln)
                assert lo == foff[i] + k * Ck and hi == foff[i] + min(dlen[i], (k + 1) * Ck), "chunks are read whole"
                read_chunks.append((i, k))
                lo = hi
        filled.sort()
        assert all(a[1] <= b[0] for a, b in zip(filled, filled[1:])), "reads overlap on the stage"
        hole_blocks, hole_bytes = r["hole"][-1]
        assert sum(b - a for a, b in filled) + hole_bytes == r["file_bytes"]

        for at, ln, pid, poff, tlen in r["lanes"]:
            assert at % BLOCK == 0 and ln > 0 and any(a <= at and at + ln <= b for a, b in filled)
            assert fed.get(pid, 0) == poff and tlen == dlen[first + pid] + pads[first + pid]
            assert poff + ln == tlen or ln % 64 == 0
            fed[pid] = poff + ln
        for pid, poff, blocks in r["runs"]:
            assert fed.get(pid, 0) == poff and poff % Ck == 0 and blocks == Ck // 64
            assert masks[first + pid][poff // Ck], "a zero run stands for a hole chunk"
            fed[pid] = poff + 64 * blocks
        # the zero runs run beside the round's lanes: they touch other pieces
        assert not {x[0] for x in r["runs"]} & {x[2] for x in r["lanes"]}
        assert len({x[0] for x in r["runs"]}) == len(r["runs"])
        chain.zero_runs(r["runs"])
        got = chain.lanes(st, r["lanes"])
        assert not set(got) & set(done1)
        done1.update(got)
        for at, dl, pad, pid in r["tails"]:
            assert pad and dl + pad == pl and at % 4 == 0 and fed.get(pid, 0) == dl & ~63
            i = first + pid
            if dl != dlen[i]:  # the trailing hole run: zeros like the pad's
                assert dl % Ck == 0 and dl < dlen[i] and all(masks[i][dl // Ck:]) and not masks[i][dl // Ck - 1]
            else:
                assert pad == pads[i] and (dl & 63 == 0 or any(a <= at and at + (dl & 63) <= b for a, b in filled))
        got = chain.tails(st, r["tails"])
        assert not set(got) & set(done1)
        done1.update(got)
        for pid, total in r["whole"]:
            i = first + pid
            assert all(masks[i]) and total == dlen[i] + pads[i] and pid not in fed
            whole[pid] = hs.sha1_of_zeros(total)  # the host's rule

        nd, nh = r["data_blocks"], hole_blocks
        table = r["table"]
        assert len(table) >= nd + nh
        rows_seen = set()
        for b, (row, ln) in enumerate(table):
            assert row < (w_n << K) and row not in leaves and row not in rows_seen
            rows_seen.add(row)
            i, slot = w_first + (row >> K), row & ((1 << K) - 1)
            assert slot < (1 << log2w[i])
            if b < nd:
                assert 0 < ln <= BLOCK and any(a <= b * BLOCK and b * BLOCK + ln <= e for a, e in filled)
                leaves[row] = hashlib.sha256(bytes(st[b * BLOCK:b * BLOCK + ln])).digest()
            elif b < len(table) - nh:
                assert ln == 0 and slot * BLOCK >= dlen[i]
                leaves[row] = bytes(32)
            else:
                assert ln == min(BLOCK, dlen[i] - slot * BLOCK) and masks[i][slot * BLOCK // Ck]
                leaves[row] = hashlib.sha256(bytes(ln)).digest()
        if r["end"]:
            for k in range(w_n):
                i = w_first + k
                done2[i - first] = _root([leaves[(k << K) + s] for s in range(1 << log2w[i])])
            next_piece, window = w_first + w_n, None
    assert window is None and next_piece == first + count
    got = chain.flush()
    assert not set(got) & set(done1)
    done1.update(got)
    assert not set(whole) & set(done1)
    done1.update(whole)
    out = []
    for pid in range(count):
        i = first + pid
        data = real[findex[i]][foff[i]:foff[i] + dlen[i]]
        assert done1.get(pid) == hybrid.v1_digest(data, pads[i]), f"{t['name']}: v1 piece {i}"
        assert done2.get(pid) == hybrid.v2_root(data, log2w[i]), f"{t['name']}: v2 piece {i}"
        out.append((done1[pid], done2[pid]))
    # no read touches a hole chunk (but the last piece's trailing run); every other chunk is read exactly once
    assert len(read_chunks) == len(set(read_chunks))
    n_all = len(dlen)
    for i in range(first, first + count):
        m = masks[i]
        t_run = len(m)
        while t_run and m[t_run - 1]:
            t_run -= 1
        must_read = i == n_all - 1 and dlen[i] < pl and 0 < t_run < len(m)
        for k, hole in enumerate(m):
            assert ((i, k) in read_chunks) == (not hole or (must_read and k >= t_run)), (i, k)
    total = sum(dlen[first:first + count])
    read = sum(ln for r in rounds for _, _, ln, _, _ in r["reads"])
    assert read + summary["hole_bytes"] == total == summary["file_bytes"]
    for key in ("hole_bytes", "hole_blocks", "hole_pieces", "zero_runs", "extents"):
        assert summary[key] == model[key], key
    assert read == model["read_bytes"]
    return rounds, summary, out


def test_no_predicate_is_todays_planner(exes, torrents):
    """With no predicate, and with one that is never true, the rounds are the
    planner's own over the same geometry, field for field."""
    new, old = exes
    for t in torrents[0].values():
        for stage, chunk, budget, first, count in ((64 << 20, 0, 0, 0, -1), (24 * BLOCK, 2 * BLOCK, 1 << 8, 0, -1),
                                                   (64 << 20, 0, 0, 1, len(t["want"]) - 1)):
            want = _lines(old, [t["pl"], first, count, stage, chunk, budget, 0],
                          "\n".join(map(str, t["flens"])) + "\n")[:-1]
            for mode in ("none", "false"):
                assert _dump(new, t, mode, stage, chunk, budget, first, count)[2] == want, (t["name"], mode, stage)


def test_layout_replayed_with_hashlib(exes, torrents):
    ts, reported = torrents
    seen, got = set(), {}
    for t in ts.values():
        # (the first replay of a torrent's files: a fallocated range that has been read can report as data)
        got[t["name"]] = rounds, s, _ = replay(exes[0], t, 64 << 20, HashlibChain(), reported)
        assert s["chunk"] == hs.C
        seen |= {k for r in rounds for k in ("runs", "whole", "tails") if r[k]}
    assert not reported or seen == {"runs", "whole", "tails"}
    # a small stage and row budget: many windows, the same digests
    a = got["main"]
    b = replay(exes[0], ts["main"], 6 * hs.C, HashlibChain(), reported, budget=1 << 8)
    assert a[2] == b[2] and b[1]["windows"] > a[1]["windows"] and b[1]["max_window_rows"] <= 1 << 8
    if not reported:
        pytest.skip(NO_HOLES)
    m = a[1]
    # file 0: 32 of its 64 chunks are holes, piece 15 wholly; the file ends' all-hole pieces; nothing of the punched piece
    assert m["hole_pieces"] == 5 and m["zero_runs"] == MAIN_ZERO_RUNS
    assert ts["last-trailing"]["want"] == [3, 3]
    lt = got["last-trailing"][1]
    assert lt["hole_bytes"] == 0 and lt["zero_runs"] == 0, "the last piece's trailing run is read"
    lw = got["last-whole"][1]
    assert lw["hole_pieces"] == 1 and lw["hole_bytes"] == 2 * hs.C + 5000
    ll = got["last-leading"][1]
    assert ll["zero_runs"] == 2 and ll["hole_pieces"] == 0 and ll["hole_bytes"] == 2 * hs.C
    sd = got["short-on-disk"][1]  # piece 0's three trailing chunks and piece 1's first; nothing at or past st_size
    assert sd["hole_bytes"] == 4 * hs.C and sd["zero_runs"] == 1 and sd["hole_pieces"] == 0
    assert got["256KiB"][1]["hole_pieces"] == 8 and got["256KiB"][1]["zero_runs"] == 0


def test_main_layout_replayed_with_the_sha1_model(exes, tmp_path):
    """The 1 MiB layout once more with the state-level model in the kernels'
    place: run_blocks for lanes, zero_blocks for zero-run lanes, zero_tail for
    tails (about 45,000 blocks in sequence)."""
    t = hs.main_torrent(tmp_path)  # (fresh files: the module's have been read, and fallocated ranges show as data then)
    reported = holes_reported(tmp_path)
    a = replay(exes[0], t, 64 << 20, ModelChain(), reported)  # (asserts every digest and root against hashlib's)
    if not reported:
        pytest.skip(NO_HOLES)
    assert a[1]["hole_pieces"] == 5 and a[1]["zero_runs"] == MAIN_ZERO_RUNS


def test_range_agrees_with_the_full_call(exes, torrents):
    """A range that starts inside file 0 (and inside a window of the full call)
    gives the pieces the full call gives them."""
    ts, reported = torrents
    t = ts["main"]
    full = replay(exes[0], t, 64 << 20, HashlibChain(), reported)[2]
    for first, count in ((5, 20), (15, 3), (44, 3)):
        assert replay(exes[0], t, 64 << 20, HashlibChain(), reported, first=first, count=count)[2] == \
            full[first:first + count]


def test_whole_hole_windows_keep_the_row_budget(exes, tmp_path):
    """4,096 unwritten pieces need no stage: the row budget and not the stage
    closes their windows, so they make few windows."""
    pl = 1 << 20
    p = tmp_path / "big"
    with open(p, "wb") as f:
        f.truncate(4096 * pl)
    t = dict(pl=pl, flens=[4096 * pl], paths=[str(p)])
    rounds, s, _ = _dump(exes[0], t, "holes", 64 << 20, budget=1 << 16)
    assert s["max_window_rows"] <= 1 << 16
    if not holes_reported(tmp_path):
        pytest.skip(NO_HOLES)
    assert s["hole_pieces"] == 4096 and s["windows"] == 4096 * 64 // (1 << 16) and s["lanes"] == s["tails"] == 0
    assert all(not r["reads"] and r["bytes"] == 0 for r in rounds)


def test_small_chunks_replayed_with_the_sha1_model(exes, tmp_path):
    """128 KiB pieces in 32 KiB chunks (the planner's chunk argument), every
    hole mask and every file end as in the 1 MiB layout, with the state-level
    model in the kernels' place."""
    rng = random.Random(12)
    pl, ck = 128 << 10, 32 << 10
    files = [hs.chunked_file(tmp_path / "m0", 16 * pl, {4 * m + j for m in range(16) for j in range(4) if m >> j & 1},
                             rng, chunk=ck)]
    for k in range(4):
        for mask in range(1 << (k + 1)):
            files.append(hs.chunked_file(tmp_path / f"e{k}_{mask}", k * ck + 4096 + 37,
                                         {j for j in range(k + 1) if mask >> j & 1}, rng, chunk=ck))
    files.append(hs.chunked_file(tmp_path / "last", pl + 2 * ck + 5000, {0, 6}, rng, chunk=ck))
    t = hs._finish("small-chunks", pl, files)
    reported = holes_reported(tmp_path)
    a = replay(exes[0], t, 64 << 20, ModelChain(), reported, chunk=ck)
    b = replay(exes[0], t, 64 << 20, HashlibChain(), reported, chunk=ck)
    assert a[2] == b[2] and a[1] == b[1]
    if not reported:
        pytest.skip(NO_HOLES)
    assert a[1]["zero_runs"] > 20 and a[1]["hole_pieces"] == 5 and a[1]["tails"] > 30
