#!/usr/bin/env python3
"""End-to-end time of the one-pass hybrid re-verify against the
two passes it replaces.

BASELINE config 5's 2,907,832,320 bytes, split into four files whose lengths
are no multiple of anything, as a hybrid (v1 + v2) torrent: page cache warm, 16
readers, piece lengths 256 KiB and 4 MiB, two legs alternating on one context:

  (a) hybrid    HashPool.verify_hybrid_files: one read and one H2D per byte, the
                pad files exist nowhere
  (b) two_pass  HashPool.verify_files over the files and materialised zero-filled
                pad files (the only way the v1 table checks on the parent tree),
                then HashPool.verify_merkle_files over the files

A call is timed with the host clock around it, after one warm-up call per leg
whose verdicts are checked against hashlib's tables; medians of --reps calls.
The claim "one pass is cheaper than two" holds when (a)'s median is below (b)'s
by more than the larger min-max spread of the two legs; the record says whether
it does, and the ratio whatever it is.  The tool exits 0 either way: the
capability (no pad files on disk) does not depend on it.

  python tools/hybrid_reverify_bench.py --out profiles/hybrid/reverify.json
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
PIECE_LENGTHS = (256 * 1024, 4 << 20)
SPLIT = (0.48, 0.31, 0.17)  # three files' shares; the fourth takes the rest
CPU_THREADS = 16
GIB = float(1 << 30)


def file_lengths(total: int) -> list:
    lens = [int(total * s) // 7 * 7 + 3 for s in SPLIT]
    return lens + [total - sum(lens)]


def write_file(path: str, n: int, seed: int) -> None:
    import numpy as np

    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        left = n
        while left:
            k = min(left, 64 << 20)
            f.write(rng.bytes(k))
            left -= k
        f.flush()
        os.fsync(f.fileno())


def expected_tables(ex, fds, flens, pl):
    """hashlib's v1 `pieces` rows and v2 roots of the hybrid torrent."""
    from vortex_amd import hybrid

    findex, foff, dlen, pads, log2w = hybrid.hybrid_pieces(flens, pl)

    def one(i):
        data = os.pread(fds[findex[i]], dlen[i], foff[i])
        return hybrid.v1_digest(data, pads[i]), hybrid.v2_root(data, log2w[i])

    both = list(ex.map(one, range(len(dlen))))
    return [a for a, _ in both], [b for _, b in both], pads


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid", "reverify.json"))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per leg and piece length (at least 5)")
    ap.add_argument("--scale", type=float, default=1.0, help="< 1 shrinks the files (rehearsal; the record says so)")
    ap.add_argument("--dir", help="where the files go (default: bench.py's choice, a disk-backed directory)")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")

    import torch

    from bench import fs_type, reverify_dir
    from vortex_amd.hash_pool import HashPool

    if not torch.cuda.is_available():
        raise SystemExit("hybrid_reverify_bench needs a GPU: a time is a measurement on the device")
    total = TOTAL if args.scale >= 1.0 else max(1 << 22, int(TOTAL * args.scale))
    flens = file_lengths(total)
    d = args.dir or reverify_dir()
    stem = os.path.join(d, f"vx_hybrid_reverify_{os.getpid()}")
    paths = [f"{stem}_{k}.bin" for k in range(len(flens))]
    made = list(paths)
    result = {"tool": "tools/hybrid_reverify_bench.py", "device": torch.cuda.get_device_properties(0).name,
              "total_bytes": total, "file_lengths": flens, "scale": args.scale, "fs": fs_type(d), "reps": args.reps,
              "io_threads": 16, "timing": "host clock around each synchronous call, page cache warm, legs "
              "alternating a, b within each repetition; medians", "piece_lengths": []}
    try:
        t0 = time.perf_counter()
        for k, (p, n) in enumerate(zip(paths, flens)):
            write_file(p, n, 0x5EED0060 + k)
        result["write_s"] = round(time.perf_counter() - t0, 2)
        fds = [os.open(p, os.O_RDONLY) for p in paths]
        with ThreadPoolExecutor(CPU_THREADS) as ex:
            for pl in PIECE_LENGTHS:
                e1, e2, pads = expected_tables(ex, fds, flens, pl)  # (also pulls the files into the page cache)
                n = len(e1)
                # leg (b)'s v1 layout: every file followed by its pad file, zeros on disk
                all_paths, all_lens, pad_bytes = [], [], 0
                for k, (p, flen) in enumerate(zip(paths, flens)):
                    all_paths.append(p)
                    all_lens.append(flen)
                    if k != len(paths) - 1 and flen % pl:
                        pp = f"{stem}_pad{k}_{pl}.bin"
                        with open(pp, "wb") as f:
                            f.write(bytes(pl - flen % pl))
                            f.flush()
                            os.fsync(f.fileno())
                        made.append(pp)
                        all_paths.append(pp)
                        all_lens.append(pl - flen % pl)
                        pad_bytes += pl - flen % pl
                b1, b2 = b"".join(e1), b"".join(e2)
                with HashPool(pl, slots=4, slot_bytes=512 << 20, batch_pieces=4096) as pool:
                    def leg_a():
                        return pool.verify_hybrid_files(paths, flens, pl, b1, b2, io_threads=16)

                    def leg_b():
                        v1, bad1 = pool.verify_files(all_paths, all_lens, pl, b1, io_threads=16)
                        v2, bad2 = pool.verify_merkle_files(paths, flens, pl, b2, io_threads=16)
                        if bad1 or bad2:
                            raise SystemExit(f"two_pass at {pl}: I/O errors")
                        return list(zip(v1, v2))

                    for name, leg in (("hybrid", leg_a), ("two_pass", leg_b)):  # warm-up, checked
                        got = leg()
                        if got != [(True, True)] * n:
                            raise SystemExit(f"{name} at {pl}: {sum(v != (True, True) for v in got)} of {n} pieces "
                                             "refused")
                    if pool.last_verify()["read_bytes"] != total:  # (the last call was leg (b)'s merkle pass)
                        raise SystemExit("verify_merkle_files did not read the files' bytes once")
                    leg_a()
                    if pool.last_verify()["read_bytes"] != total:
                        raise SystemExit("verify_hybrid_files did not read the files' bytes once")
                    # ... and a wrong row of each table is seen, on its own bit
                    w1, w2 = bytearray(b1), bytearray(b2)
                    w1[20 * (n // 2)] ^= 1
                    w2[32 * (n // 3)] ^= 1
                    got = pool.verify_hybrid_files(paths, flens, pl, bytes(w1), bytes(w2), io_threads=16)
                    want = [(i != n // 2, i != n // 3) for i in range(n)]
                    if got != want:
                        raise SystemExit(f"hybrid at {pl}: wrong expected rows were not the bits refused")
                    times = {"hybrid": [], "two_pass": []}
                    traces = []
                    for _ in range(args.reps):
                        for name, leg in (("hybrid", leg_a), ("two_pass", leg_b)):
                            t0 = time.perf_counter()
                            leg()
                            times[name].append(time.perf_counter() - t0)
                            if name == "hybrid":
                                traces.append(pool.last_verify())
                rec = {"piece_length": pl, "pieces": n, "padded_pieces": sum(1 for x in pads if x),
                       "pad_bytes_on_disk_for_two_pass": pad_bytes}
                for name, ts in times.items():
                    med = statistics.median(ts)
                    rec[name] = {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                                 "spread_s": round(max(ts) - min(ts), 5), "GiB_per_s": round(total / GIB / med, 2),
                                 "calls_s": [round(t, 5) for t in ts]}
                k = sorted(range(len(times["hybrid"])), key=lambda i: times["hybrid"][i])[len(traces) // 2]
                rec["hybrid"]["last_verify_of_median"] = {
                    key: (round(v, 3) if isinstance(v, float) else v) for key, v in traces[k].items()}
                gap = rec["two_pass"]["median_s"] - rec["hybrid"]["median_s"]
                spread = max(rec["hybrid"]["spread_s"], rec["two_pass"]["spread_s"])
                rec["two_pass_over_hybrid"] = round(rec["two_pass"]["median_s"] / rec["hybrid"]["median_s"], 3)
                rec["claim_one_pass_is_cheaper"] = {"median_gap_s": round(gap, 5), "larger_spread_s": round(spread, 5),
                                                    "holds": gap > spread}
                result["piece_lengths"].append(rec)
                print(json.dumps({k: v for k, v in rec.items()}), flush=True)
        for fd in fds:
            os.close(fd)
    finally:
        for p in made:
            if os.path.exists(p):
                os.unlink(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
