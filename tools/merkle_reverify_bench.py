#!/usr/bin/env python3
"""End-to-end rate of the BitTorrent v2 re-verify from disk.

One file of BASELINE config 5's size (2,907,832,320 bytes), page cache warm,
re-verified at piece lengths 256 KiB, 4 MiB and 16 MiB by three legs that
alternate within this one process:

  (a) merkle_files  HashPool.verify_merkle_files (v2: rounds of 16 KiB blocks)
  (b) sha1_files    HashPool.verify_files (v1: SHA-1, one chain per piece) on the
                    same file, pool and piece length
  (c) cpu_v2        16 threads of pread + hashlib.sha256 building the same trees:
                    what a client runs without the engine; recorded for context

A call is timed with the host clock around it (every leg returns after its last
verdict is on the host), after one warm-up call per leg whose verdicts are
checked; medians of --reps calls are reported, with (a)'s and (b)'s
last_verify() of the median call.

One condition: at 16 MiB pieces (a) >= 2 x (b).  (b)'s last piece is one chain
of 262,144 blocks that cannot finish before its bytes arrive; (a) has no chain.
The ratio is recorded at every piece length and the tool exits 1 if the
condition fails.

  python tools/merkle_reverify_bench.py --out profiles/merkle/reverify.json
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
PIECE_LENGTHS = (256 * 1024, 4 << 20, 16 << 20)
CPU_THREADS = 16
GIB = float(1 << 30)


def write_file(path: str, total: int) -> None:
    import numpy as np

    rng = np.random.default_rng(0x5EED0052)
    with open(path, "wb") as f:
        left = total
        while left:
            n = min(left, 64 << 20)
            f.write(rng.bytes(n))
            left -= n
        f.flush()
        os.fsync(f.fileno())  # writeback done before anything is timed


def v2_piece_root(fd: int, off: int, length: int, log2w: int) -> bytes:
    data = os.pread(fd, length, off)
    rows = [hashlib.sha256(data[o:o + BLOCK]).digest() for o in range(0, len(data), BLOCK)]
    rows += [bytes(32)] * ((1 << log2w) - len(rows))
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


def cpu_v2(ex: ThreadPoolExecutor, fd: int, total: int, pl: int) -> list:
    """Leg (c): the roots of every piece of the one file, piece per task."""
    from vortex_amd import merkle

    lens, log2w = merkle.file_pieces(total, pl)
    return list(ex.map(lambda i: v2_piece_root(fd, i * pl, lens[i], log2w[i]), range(len(lens))))


def cpu_sha1(ex: ThreadPoolExecutor, fd: int, total: int, pl: int) -> list:
    n = -(-total // pl)
    return list(ex.map(lambda i: hashlib.sha1(os.pread(fd, min(pl, total - i * pl), i * pl)).digest(), range(n)))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "reverify.json"))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per leg and piece length (at least 5)")
    ap.add_argument("--scale", type=float, default=1.0, help="< 1 shrinks the file (rehearsal; the record says so)")
    ap.add_argument("--dir", help="where the file goes (default: bench.py's choice, a disk-backed directory)")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")

    import torch

    from bench import fs_type, reverify_dir
    from vortex_amd.hash_pool import HashPool

    if not torch.cuda.is_available():
        raise SystemExit("merkle_reverify_bench needs a GPU: a rate is a measurement on the device")
    total = TOTAL if args.scale >= 1.0 else max(BLOCK, int(TOTAL * args.scale))
    d = args.dir or reverify_dir()
    path = os.path.join(d, f"vx_merkle_reverify_{os.getpid()}.bin")
    result = {"tool": "tools/merkle_reverify_bench.py", "device": torch.cuda.get_device_properties(0).name,
              "file_bytes": total, "scale": args.scale, "fs": fs_type(d), "reps": args.reps,
              "cpu_threads": CPU_THREADS, "timing": "host clock around each synchronous call, page cache warm, "
              "legs alternating a, b, c within each repetition; medians", "piece_lengths": []}
    ok = True
    try:
        t0 = time.perf_counter()
        write_file(path, total)
        result["write_s"] = round(time.perf_counter() - t0, 2)
        fd = os.open(path, os.O_RDONLY)
        with ThreadPoolExecutor(CPU_THREADS) as ex:
            for pl in PIECE_LENGTHS:
                exp2 = cpu_v2(ex, fd, total, pl)   # (also pulls the file into the page cache)
                exp1 = cpu_sha1(ex, fd, total, pl)
                n = len(exp1)
                assert len(exp2) == n
                e2, e1 = b"".join(exp2), b"".join(exp1)
                with HashPool(pl, slots=4, slot_bytes=512 << 20, batch_pieces=4096) as pool:
                    def leg_a():
                        return pool.verify_merkle_files([path], [total], pl, e2, io_threads=16)

                    def leg_b():
                        return pool.verify_files([path], [total], pl, e1, io_threads=16)

                    def leg_c():
                        return cpu_v2(ex, fd, total, pl)

                    for name, leg in (("merkle_files", leg_a), ("sha1_files", leg_b)):  # warm-up, checked
                        got, bad = leg()
                        if bad or not all(got) or len(got) != n:
                            raise SystemExit(f"{name} at {pl}: {got.count(False)} of {n} verdicts false, "
                                             f"{bad} I/O errors")
                    # ... and a wrong row is seen
                    wrong = bytearray(e2)
                    wrong[32 * (n // 2)] ^= 1
                    got, _ = pool.verify_merkle_files([path], [total], pl, bytes(wrong), io_threads=16)
                    if [i for i, v in enumerate(got) if not v] != [n // 2]:
                        raise SystemExit(f"merkle_files at {pl}: a wrong expected row was not the one piece refused")
                    if leg_c() != exp2:
                        raise SystemExit("cpu_v2 is not repeatable")
                    times = {"merkle_files": [], "sha1_files": [], "cpu_v2": []}
                    traces = {"merkle_files": [], "sha1_files": []}
                    for _ in range(args.reps):
                        for name, leg in (("merkle_files", leg_a), ("sha1_files", leg_b), ("cpu_v2", leg_c)):
                            t0 = time.perf_counter()
                            leg()
                            times[name].append(time.perf_counter() - t0)
                            if name in traces:
                                traces[name].append(pool.last_verify())
                rec = {"piece_length": pl, "pieces": n}
                for name, ts in times.items():
                    med = statistics.median(ts)
                    rates = sorted(total / GIB / t for t in ts)
                    rec[name] = {"median_s": round(med, 5), "GiB_per_s": round(total / GIB / med, 2),
                                 "GiB_per_s_min": round(rates[0], 2), "GiB_per_s_max": round(rates[-1], 2),
                                 "calls_s": [round(t, 5) for t in ts]}
                    if name in traces:
                        k = sorted(range(len(ts)), key=lambda i: ts[i])[len(ts) // 2]
                        rec[name]["last_verify_of_median"] = {
                            key: (round(v, 3) if isinstance(v, float) else v) for key, v in traces[name][k].items()}
                rec["merkle_over_sha1"] = round(rec["merkle_files"]["GiB_per_s"] / rec["sha1_files"]["GiB_per_s"], 3)
                rec["merkle_over_cpu_v2"] = round(rec["merkle_files"]["GiB_per_s"] / rec["cpu_v2"]["GiB_per_s"], 3)
                if pl == 16 << 20:
                    rec["condition"] = {"merkle_over_sha1_min": 2.0, "met": rec["merkle_over_sha1"] >= 2.0}
                    ok = ok and rec["condition"]["met"]
                result["piece_lengths"].append(rec)
                print(json.dumps({k: v for k, v in rec.items() if k != "calls_s"}), flush=True)
        os.close(fd)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        print("verify_merkle_files is under 2x verify_files at 16 MiB pieces", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
