#!/usr/bin/env python3
"""What skipping file holes saves the re-verify.

One fallocated file of BASELINE config 5's geometry (2,907,832,320 bytes,
2 MiB pieces) in three states of a download:

  0 %    nothing written: what the reference re-verifies right after
         FileStore::new (file_store.rs:146)
  50 %   alternating runs of 64 pieces written
  100 %  every piece written

For each state, v1 (HashPool.verify_files) and v2 (verify_merkle_files) run
with skip_holes off and on, alternating within this one process, at least 7
calls each.  The off legs are the yardstick: what the engine did before.  Per
leg the record keeps the calls' times (host clock around each synchronous
call; median, min, max), read_bytes, the hole trace of the median call and
whether the verdicts of off and on are equal (and what the state says they
must be).  The first `on` call of the context is kept apart: it alone makes
the zero digest of a 2 MiB piece (32,769 chained blocks).

Before every call, off or on, the ranges not yet written are dropped from the
page cache (posix_fadvise DONTNEED): on ext4 a fallocated range that has been
read through the page cache reports as data while its pages stay cached, and
an `off` leg's buffered reads would otherwise hide the holes from the `on` leg
that follows.  A client's resume starts with none of that cached.

The hybrid legs (--legs hybrid; HashPool.verify_hybrid_files, where the unit
is the 256 KiB chunk) run the same bytes as four fallocated files, at 256 KiB
and at 4 MiB pieces, in the same three states and in a fourth, every piece half
written (alternate chunks; at 256 KiB pieces a piece is one chunk, so alternate
pieces), whose expected tables are those of what the files then hold.  Off and
on alternate in one process as above.  Each leg is held to §6.11's rule: at
100 % the `on` median lies inside the `off` calls' min-max, elsewhere `on` is
below `off` by more than the larger of the two spreads.  Beside them, the
zero-run kernel's time per zero block and the zero-tail kernel's, from the same
process.  Their record is added to the output file under "hybrid"; what the
file held before stays.

  python tools/sparse_reverify_bench.py --out profiles/sparse/reverify.json
  python tools/sparse_reverify_bench.py --legs hybrid --out profiles/sparse/reverify.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BLOCK = 16384
TOTAL = 2907832320
PL = 2 << 20
RUN = 64  # pieces per written / unwritten run of the 50 % state
THREADS = 16


def piece_bytes(i: int, n: int) -> bytes:
    import numpy as np

    return np.random.default_rng(0x5A125E + i).bytes(n)


def v2_root(data: bytes, log2w: int) -> bytes:
    rows = [hashlib.sha256(data[o:o + BLOCK]).digest() for o in range(0, len(data), BLOCK)]
    rows += [bytes(32)] * ((1 << log2w) - len(rows))
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


def stats(ts_ms: list) -> dict:
    return {"median_ms": round(statistics.median(ts_ms), 3), "min_ms": round(min(ts_ms), 3),
            "max_ms": round(max(ts_ms), 3), "calls_ms": [round(t, 3) for t in ts_ms]}


HYBRID_PIECES = (256 << 10, 4 << 20)


def zero_kernels_per_block(torch, lanes: int = 1024, blocks: int = 4096, reps: int = 7) -> dict:
    """The zero-run kernel's and the zero-tail kernel's time per zero block (one
    launch of `lanes` lanes of `blocks` blocks each, device events, median)."""
    from vortex_amd._lib import check, tuning

    dev = torch.device("cuda:0")
    T = tuning()
    i32 = dict(dtype=torch.int32, device=dev)
    states = torch.randint(0, 1 << 31, (lanes, 5), **i32)
    pids, poffs = torch.arange(lanes, **i32), torch.full((lanes,), 64, **i32)
    nblk = torch.full((lanes,), blocks, **i32)
    pl = 64 * (blocks + 1)  # the tail's piece: one data block, then `blocks` blocks of pad
    lens, pads = torch.full((lanes,), 64, **i32), torch.full((lanes,), 64 * blocks, **i32)
    offs = torch.zeros(lanes, dtype=torch.int64, device=dev)
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    dig = torch.zeros((lanes, 20), dtype=torch.uint8, device=dev)
    sp = int(torch.cuda.current_stream(dev).cuda_stream)
    legs = {
        "zero_run": lambda: check(T.vx_tuning_zero_run_kernel(pids.data_ptr(), poffs.data_ptr(), nblk.data_ptr(), lanes,
                                                              states.data_ptr(), sp), "vx_tuning_zero_run_kernel", T),
        "zero_tail": lambda: check(T.vx_tuning_zero_tail_kernel(buf.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                                                pads.data_ptr(), lanes, pl, states.data_ptr(),
                                                                dig.data_ptr(), sp), "vx_tuning_zero_tail_kernel", T),
    }
    ms = {k: [] for k in legs}
    for r in range(reps + 1):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r:  # (the first round warms up)
                ms[name].append(a.elapsed_time(b))
    out = {"lanes": lanes, "blocks_per_lane": blocks, "reps": reps,
           "timing": "device events around one launch, ms; the two kernels alternate"}
    for name, ts in ms.items():
        out[name] = dict(stats(ts), us_per_block=round(statistics.median(ts) * 1e3 / blocks, 4))
    return out


def hybrid_legs(args, torch) -> tuple[dict, bool]:
    """The "hybrid" record (see the module's text) and whether every leg's verdicts were equal off and on."""
    from bench import fs_type, reverify_dir
    from vortex_amd import hybrid, sparse
    from vortex_amd.hash_pool import HashPool

    total = TOTAL if args.scale >= 1.0 else max(4 * (4 << 20) + 4, int(TOTAL * args.scale))
    q = total // 4
    flens = [q + 12345, q - 777, q + 1, total - 3 * q - 12345 + 777 - 1]
    d = args.dir or reverify_dir()
    paths = [os.path.join(d, f"vx_sparse_hybrid_{os.getpid()}_{k}.bin") for k in range(4)]
    rec = {"files": flens, "fs": fs_type(d), "reps": args.reps, "scale": args.scale, "piece_lengths": []}
    ok = True

    def fresh():
        for p, n in zip(paths, flens):
            if os.path.exists(p):
                os.unlink(p)
            with open(p, "wb") as f:
                os.posix_fallocate(f.fileno(), 0, n)

    try:
        with ThreadPoolExecutor(THREADS) as ex:
            for pl in HYBRID_PIECES:
                findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(flens, pl)
                n, C = len(dlen), sparse.hybrid_chunk(pl)
                nck = [-(-x // C) for x in dlen]

                def half_kept(i, k):  # the chunks the half-written state holds
                    return (k if nck[i] > 1 else i) % 2 == 0

                def content(i, half):
                    b = piece_bytes(i, dlen[i])
                    if half:
                        b = b"".join(b[k * C:(k + 1) * C] if half_kept(i, k) else bytes(len(b[k * C:(k + 1) * C]))
                                     for k in range(nck[i]))
                    return b

                def tables(half):
                    rows = list(ex.map(lambda i: (lambda b: (hybrid.v1_digest(b, pads[i]), hybrid.v2_root(b, log2w[i])))(
                        content(i, half)), range(n)))
                    return b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)

                t0 = time.perf_counter()
                full_tables, half_tables = tables(False), tables(True)
                prec = {"piece_length": pl, "pieces": n, "chunk": C,
                        "expected_tables_s": round(time.perf_counter() - t0, 2), "states": []}
                written: set = set()  # (piece, chunk)

                def write(chunks):
                    def one(ik):
                        i, k = ik
                        fd = os.open(paths[findex[i]], os.O_WRONLY)
                        try:
                            os.pwrite(fd, piece_bytes(i, dlen[i])[k * C:(k + 1) * C], foff[i] + k * C)
                        finally:
                            os.close(fd)
                    list(ex.map(one, chunks))
                    for p in paths:
                        fd = os.open(p, os.O_RDONLY)
                        os.fsync(fd)
                        os.close(fd)
                    written.update(chunks)

                def drop_unwritten(fds):
                    run = None  # (file, lo, hi) of adjacent unwritten chunks
                    for i in range(n):
                        for k in range(nck[i]):
                            lo = foff[i] + k * C
                            hi = foff[i] + min(dlen[i], (k + 1) * C)
                            if (i, k) in written:
                                continue
                            if run and run[0] == findex[i] and run[2] == lo:
                                run = (run[0], run[1], hi)
                                continue
                            if run:
                                os.posix_fadvise(fds[run[0]], run[1], run[2] - run[1], os.POSIX_FADV_DONTNEED)
                            run = (findex[i], lo, hi)
                    if run:
                        os.posix_fadvise(fds[run[0]], run[1], run[2] - run[1], os.POSIX_FADV_DONTNEED)

                def chunks_of(pieces):
                    return [(i, k) for i in pieces for k in range(nck[i])]

                with HashPool(pl, slots=4, slot_bytes=512 << 20, batch_pieces=4096) as pool:
                    seen_on = False
                    for state in ("0", "50", "100", "half"):
                        if state in ("0", "half"):
                            fresh()
                            written.clear()
                        if state == "50":
                            write(chunks_of(i for i in range(n) if (i // RUN) % 2 == 0))
                        elif state == "100":
                            write(chunks_of(i for i in range(n) if (i // RUN) % 2 == 1))
                        elif state == "half":
                            write([(i, k) for i in range(n) for k in range(nck[i]) if half_kept(i, k)])
                        e1, e2 = half_tables if state == "half" else full_tables
                        if state == "half":
                            want = [(True, True)] * n
                        else:
                            want = [((i, 0) in written,) * 2 for i in range(n)]
                        fds = [os.open(p, os.O_RDONLY) for p in paths]
                        try:
                            drop_unwritten(fds)
                            model = sparse.hybrid_read_bytes(paths, flens, pl)
                            leg = lambda: pool.verify_hybrid_files(paths, flens, pl, e1, e2, io_threads=THREADS)  # noqa: E731
                            pool.skip_holes = False
                            warm = leg()
                            if warm != want:
                                raise SystemExit(f"hybrid at {pl} bytes, {state}: verdicts differ from the state's")
                            out = {"state": state, "written_bytes": sum(
                                min(dlen[i], (k + 1) * C) - k * C for i, k in written), "model": model}
                            if not seen_on and state != "100":  # the context's first call over holes makes the zero hashes
                                pool.skip_holes = True
                                drop_unwritten(fds)
                                t0 = time.perf_counter()
                                got = leg()
                                out["first_on_call"] = {"call_ms": round((time.perf_counter() - t0) * 1e3, 3),
                                                        "holes": pool.last_verify_holes(), "verdicts_equal": got == warm}
                                seen_on = True
                            times, traces, equal = {"off": [], "on": []}, {"off": [], "on": []}, True
                            for _ in range(args.reps):
                                res = {}
                                for mode in ("off", "on"):
                                    pool.skip_holes = mode == "on"
                                    drop_unwritten(fds)
                                    t0 = time.perf_counter()
                                    res[mode] = leg()
                                    times[mode].append((time.perf_counter() - t0) * 1e3)
                                    traces[mode].append((pool.last_verify(), pool.last_verify_holes()))
                                equal = equal and res["on"] == res["off"] == want
                        finally:
                            for fd in fds:
                                os.close(fd)
                        out["verdicts_equal"] = equal
                        ok = ok and equal
                        for mode in ("off", "on"):
                            ts = times[mode]
                            k = sorted(range(len(ts)), key=lambda j: ts[j])[len(ts) // 2]
                            lv, holes_tr = traces[mode][k]
                            out[mode] = dict(stats(ts), read_bytes=lv["read_bytes"], copy_bytes=lv["copy_bytes"],
                                             rounds=lv["rounds"],
                                             holes={key: (round(v, 3) if isinstance(v, float) else v)
                                                    for key, v in holes_tr.items()})
                        off, on = out["off"], out["on"]
                        out["on_over_off"] = round(on["median_ms"] / off["median_ms"], 4)
                        spread = max(off["max_ms"] - off["min_ms"], on["max_ms"] - on["min_ms"])
                        if state == "100":
                            out["rule"] = {"text": "on median inside off min-max",
                                           "holds": off["min_ms"] <= on["median_ms"] <= off["max_ms"]}
                        else:
                            out["rule"] = {"text": "off median - on median > larger spread",
                                           "larger_spread_ms": round(spread, 3),
                                           "holds": off["median_ms"] - on["median_ms"] > spread}
                        prec["states"].append(out)
                        print(json.dumps({"hybrid_piece_length": pl, "state": state, "off_ms": off["median_ms"],
                                          "on_ms": on["median_ms"], "read_off": off["read_bytes"],
                                          "read_on": on["read_bytes"], "equal": equal, "rule": out["rule"]["holds"]}),
                              flush=True)
                rec["piece_lengths"].append(prec)
        rec["zero_kernels"] = zero_kernels_per_block(torch)
        print(json.dumps({"zero_kernels": {k: v["us_per_block"] for k, v in rec["zero_kernels"].items()
                                           if isinstance(v, dict)}}), flush=True)
    finally:
        for p in paths:
            if os.path.exists(p):
                os.unlink(p)
    return rec, ok


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse", "reverify.json"))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per leg (at least 7)")
    ap.add_argument("--scale", type=float, default=1.0, help="< 1 shrinks the file (rehearsal; the record says so)")
    ap.add_argument("--dir", help="where the file goes (default: bench.py's choice, a disk-backed directory)")
    ap.add_argument("--legs", choices=("v1v2", "hybrid"), default="v1v2",
                    help="hybrid: the hybrid legs only, added to --out's record under \"hybrid\"")
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")

    import torch

    if args.legs == "hybrid":
        if not torch.cuda.is_available():
            raise SystemExit("sparse_reverify_bench needs a GPU: a time is a measurement on the device")
        rec, ok = hybrid_legs(args, torch)
        rec["device"] = torch.cuda.get_device_properties(0).name
        result = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                result = json.load(f)
        result["hybrid"] = rec
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        if not ok:
            print("verdicts with skip_holes on differ from those with it off", file=sys.stderr)
        return 0 if ok else 1

    from bench import fs_type, reverify_dir
    from vortex_amd import merkle, sparse
    from vortex_amd.hash_pool import HashPool

    if not torch.cuda.is_available():
        raise SystemExit("sparse_reverify_bench needs a GPU: a time is a measurement on the device")
    total = TOTAL if args.scale >= 1.0 else max(PL + 1, int(TOTAL * args.scale))
    n = -(-total // PL)
    plen = [min(PL, total - i * PL) for i in range(n)]
    d = args.dir or reverify_dir()
    path = os.path.join(d, f"vx_sparse_reverify_{os.getpid()}.bin")
    result = {"tool": "tools/sparse_reverify_bench.py", "device": torch.cuda.get_device_properties(0).name,
              "file_bytes": total, "piece_length": PL, "pieces": n, "scale": args.scale, "fs": fs_type(d),
              "reps": args.reps, "timing": "host clock around each synchronous call, ms; off and on alternate "
              "within each repetition; unwritten ranges dropped from the page cache before every call", "states": []}
    _, log2w = merkle.file_pieces(total, PL)
    ok = True
    try:
        with open(path, "wb") as f:
            os.posix_fallocate(f.fileno(), 0, total)
        with ThreadPoolExecutor(THREADS) as ex:
            t0 = time.perf_counter()
            rows = list(ex.map(lambda i: (lambda b: (hashlib.sha1(b).digest(), v2_root(b, log2w[i])))(
                piece_bytes(i, plen[i])), range(n)))
            result["expected_tables_s"] = round(time.perf_counter() - t0, 2)
            e1, e2 = b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
            written: set = set()

            def write(pieces):
                def one(i):
                    fd = os.open(path, os.O_WRONLY)
                    try:
                        os.pwrite(fd, piece_bytes(i, plen[i]), i * PL)
                    finally:
                        os.close(fd)
                list(ex.map(one, pieces))
                fd = os.open(path, os.O_RDONLY)
                os.fsync(fd)  # writeback done before anything is timed
                os.close(fd)
                written.update(pieces)

            with HashPool(PL, slots=4, slot_bytes=512 << 20, batch_pieces=4096) as pool:
                fd_adv = os.open(path, os.O_RDONLY)

                def drop_unwritten():
                    i = 0
                    while i < n:
                        if i in written:
                            i += 1
                            continue
                        j = i
                        while j < n and j not in written:
                            j += 1
                        os.posix_fadvise(fd_adv, i * PL, min(total, j * PL) - i * PL, os.POSIX_FADV_DONTNEED)
                        i = j

                legs = {"v1": lambda: pool.verify_files([path], [total], PL, e1, io_threads=THREADS),
                        "v2": lambda: pool.verify_merkle_files([path], [total], PL, e2, io_threads=THREADS)}
                first_on = {}
                for state, pieces in (("0", []), ("50", [i for i in range(n) if (i // RUN) % 2 == 0]),
                                      ("100", [i for i in range(n) if (i // RUN) % 2 == 1])):
                    write(pieces)
                    want = [i in written for i in range(n)]
                    rec = {"written_percent": int(state), "written_pieces": len(written),
                           "written_bytes": sum(plen[i] for i in written)}
                    holes, extents = sparse.hole_pieces([path], [total], PL)
                    rec["model"] = {"hole_pieces": sum(holes), "extents": extents}
                    for name, leg in legs.items():
                        pool.skip_holes = False
                        drop_unwritten()
                        warm = leg()  # warm-up, checked: stages, rows, the written data in the page cache
                        if warm != (want, 0):
                            raise SystemExit(f"{name} at {state} %: verdicts differ from the state's")
                        if name not in first_on:  # the context's first call over holes: it makes the zero hashes
                            pool.skip_holes = True
                            drop_unwritten()
                            t0 = time.perf_counter()
                            got = leg()
                            first_on[name] = {"state_percent": int(state),
                                              "call_ms": round((time.perf_counter() - t0) * 1e3, 3),
                                              "holes": pool.last_verify_holes(), "verdicts_equal": got == warm}
                        times = {"off": [], "on": []}
                        traces = {"off": [], "on": []}
                        equal = True
                        for _ in range(args.reps):
                            res = {}
                            for mode in ("off", "on"):
                                pool.skip_holes = mode == "on"
                                drop_unwritten()
                                t0 = time.perf_counter()
                                res[mode] = leg()
                                times[mode].append((time.perf_counter() - t0) * 1e3)
                                traces[mode].append((pool.last_verify(), pool.last_verify_holes()))
                            equal = equal and res["on"] == res["off"] == (want, 0)
                        out = {"verdicts_equal": equal}
                        ok = ok and equal
                        for mode in ("off", "on"):
                            ts = times[mode]
                            k = sorted(range(len(ts)), key=lambda i: ts[i])[len(ts) // 2]
                            lv, holes_tr = traces[mode][k]
                            out[mode] = dict(stats(ts), read_bytes=lv["read_bytes"], copy_bytes=lv["copy_bytes"],
                                             holes={key: (round(v, 3) if isinstance(v, float) else v)
                                                    for key, v in holes_tr.items()})
                        out["on_over_off"] = round(out["on"]["median_ms"] / out["off"]["median_ms"], 4)
                        rec[name] = out
                        print(json.dumps({"state": state, "leg": name, "off_ms": out["off"]["median_ms"],
                                          "on_ms": out["on"]["median_ms"], "read_off": out["off"]["read_bytes"],
                                          "read_on": out["on"]["read_bytes"], "equal": equal}), flush=True)
                    result["states"].append(rec)
                result["first_on_call"] = first_on
                os.close(fd_adv)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        print("verdicts with skip_holes on differ from those with it off", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
