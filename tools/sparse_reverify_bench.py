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

  python tools/sparse_reverify_bench.py --out profiles/sparse/reverify.json
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse", "reverify.json"))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per leg (at least 7)")
    ap.add_argument("--scale", type=float, default=1.0, help="< 1 shrinks the file (rehearsal; the record says so)")
    ap.add_argument("--dir", help="where the file goes (default: bench.py's choice, a disk-backed directory)")
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")

    import torch

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
