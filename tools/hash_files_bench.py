#!/usr/bin/env python3
"""What hashing files into torrent metadata costs: each
hash_*_files call beside the verify_*_files call of its kind, beside a 16-thread
hashlib pool building the same tables, and build_piece_trees beside
merkle.build_tree.

BASELINE config 5's file of 2,907,832,320 bytes, page cache warm, 16 readers,
piece lengths 256 KiB and 4 MiB.  Per kind (v1, v2, hybrid) two legs alternate
on one context within each repetition:

  (a) hash     HashPool.hash_files / hash_merkle_files / hash_hybrid_files
  (b) verify   HashPool.verify_files / verify_merkle_files / verify_hybrid_files
               over the tables leg (a) returned

and a pool of 16 threads builds the same tables with hashlib (v2 and hybrid:
the piece rows and the file's tree), a few times.  The rounds of (a) and (b) are
the same; (a) brings 20-32 bytes per piece back and runs the tree passes.  A
call is timed with the host clock around it after one warm-up call per leg whose
output is checked against hashlib's tables; medians of --reps calls.  The record
holds the ratio hash / verify per kind and piece length and says whether the gap
exceeds the verify leg's own min-max spread in the same alternation; if it does,
the trace of the median hash call (vx_last_verify) beside the verify call's
shows where the time goes.  The tool exits 0 either way: this is a record, not a
gate.

Trees alone: build_piece_trees over one layer of 4 M rows and over 100,000 small
layers (counts 1..64), against merkle.build_tree on one thread; and the
engine's call alone (vx_merkle_build_trees on buffers made once), since the
Python wrapper cuts the result into one bytes object per layer.

  python tools/hash_files_bench.py --out profiles/create/hash_files.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOTAL = 2907832320
PIECE_LENGTHS = (256 * 1024, 4 << 20)
CPU_THREADS = 16
GIB = float(1 << 30)


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


def summary(ts, total=None):
    med = statistics.median(ts)
    out = {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
           "spread_s": round(max(ts) - min(ts), 5), "calls_s": [round(t, 5) for t in ts]}
    if total:
        out["GiB_per_s"] = round(total / GIB / med, 2)
    return out


def rounded(trace):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in trace.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "create", "hash_files.json"))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per leg (at least 5)")
    ap.add_argument("--cpu-reps", type=int, default=3, help="timed runs of the hashlib pool per kind")
    ap.add_argument("--scale", type=float, default=1.0, help="< 1 shrinks the file (rehearsal; the record says so)")
    ap.add_argument("--dir", help="where the file goes (default: bench.py's choice, a disk-backed directory)")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")

    import torch

    from bench import fs_type, reverify_dir
    from vortex_amd import hybrid, merkle
    from vortex_amd.hash_pool import HashPool

    if not torch.cuda.is_available():
        raise SystemExit("hash_files_bench needs a GPU: a time is a measurement on the device")
    total = TOTAL if args.scale >= 1.0 else max(1 << 22, int(TOTAL * args.scale))
    d = args.dir or reverify_dir()
    path = os.path.join(d, f"vx_hash_files_{os.getpid()}.bin")
    paths, flens = [path], [total]
    result = {"tool": "tools/hash_files_bench.py", "device": torch.cuda.get_device_properties(0).name,
              "total_bytes": total, "scale": args.scale, "fs": fs_type(d), "reps": args.reps, "io_threads": 16,
              "cpu_threads": CPU_THREADS,
              "timing": "host clock around each synchronous call, page cache warm, legs alternating hash, verify "
                        "within each repetition; medians", "piece_lengths": [], "trees": []}
    try:
        t0 = time.perf_counter()
        write_file(path, total, 0x5EED0070)
        result["write_s"] = round(time.perf_counter() - t0, 2)
        fd = os.open(path, os.O_RDONLY)
        with ThreadPoolExecutor(CPU_THREADS) as ex:
            for pl in PIECE_LENGTHS:
                n = (total + pl - 1) // pl
                _, _, dlen, pads, lw = hybrid.hybrid_pieces(flens, pl)
                height = merkle.log2_width(pl)

                # the 16-thread pool's three jobs: the same tables with hashlib
                def cpu_v1():
                    return b"".join(ex.map(lambda i: hashlib.sha1(os.pread(fd, pl, i * pl)).digest(), range(n)))

                def cpu_v2():
                    rows = list(ex.map(lambda i: hybrid.v2_root(os.pread(fd, dlen[i], i * pl), lw[i]), range(n)))
                    return b"".join(rows), (merkle.build_tree(rows, height) if n > 1 else rows[0])

                def cpu_hybrid():
                    def one(i):
                        data = os.pread(fd, dlen[i], i * pl)
                        return hybrid.v1_digest(data, pads[i]), hybrid.v2_root(data, lw[i])

                    both = list(ex.map(one, range(n)))
                    rows = [b for _, b in both]
                    return (b"".join(a for a, _ in both), b"".join(rows),
                            merkle.build_tree(rows, height) if n > 1 else rows[0])

                want_v1 = cpu_v1()  # (also pulls the file into the page cache)
                want_rows, want_tree = cpu_v2()
                want_h1, _, _ = cpu_hybrid()
                rec = {"piece_length": pl, "pieces": n, "tree_rows": merkle.tree_rows(n)}
                with HashPool(pl, slots=4, slot_bytes=512 << 20, batch_pieces=4096) as pool:
                    kinds = {
                        "v1": (lambda: pool.hash_files(paths, flens, pl, io_threads=16),
                               lambda: pool.verify_files(paths, flens, pl, want_v1, io_threads=16), cpu_v1),
                        "v2": (lambda: pool.hash_merkle_files(paths, flens, pl, io_threads=16),
                               lambda: pool.verify_merkle_files(paths, flens, pl, want_rows, io_threads=16), cpu_v2),
                        "hybrid": (lambda: pool.hash_hybrid_files(paths, flens, pl, io_threads=16),
                                   lambda: pool.verify_hybrid_files(paths, flens, pl, want_h1, want_rows,
                                                                    io_threads=16), cpu_hybrid),
                    }
                    for kind, (hash_leg, verify_leg, cpu_leg) in kinds.items():
                        got = hash_leg()  # warm-up, checked against hashlib's tables
                        want = {"v1": (want_v1, [True] * n, 0), "v2": (want_rows, [True] * n, want_tree, 0),
                                "hybrid": (want_h1, want_rows, [True] * n, want_tree, 0)}[kind]
                        if got != want:
                            raise SystemExit(f"{kind} at {pl}: the hash call's tables differ from hashlib's")
                        ok = verify_leg()
                        flat = ok[0] if kind != "hybrid" else [a and b for a, b in ok]
                        if not all(flat):
                            raise SystemExit(f"{kind} at {pl}: the verify call refused pieces")
                        times = {"hash": [], "verify": []}
                        traces = {"hash": [], "verify": []}
                        for _ in range(args.reps):
                            for name, leg in (("hash", hash_leg), ("verify", verify_leg)):
                                t0 = time.perf_counter()
                                leg()
                                times[name].append(time.perf_counter() - t0)
                                traces[name].append(pool.last_verify())
                        cpu_ts = []
                        for _ in range(args.cpu_reps):
                            t0 = time.perf_counter()
                            cpu_leg()
                            cpu_ts.append(time.perf_counter() - t0)
                        k = {"hash": summary(times["hash"], total), "verify": summary(times["verify"], total),
                             "hashlib_pool": summary(cpu_ts, total)}
                        gap = k["hash"]["median_s"] - k["verify"]["median_s"]
                        k["hash_over_verify"] = round(k["hash"]["median_s"] / k["verify"]["median_s"], 3)
                        k["hashlib_pool_over_hash"] = round(k["hashlib_pool"]["median_s"] / k["hash"]["median_s"], 2)
                        k["hash_slower_than_verify_spread"] = {"median_gap_s": round(gap, 5),
                                                               "verify_spread_s": k["verify"]["spread_s"],
                                                               "holds": gap > k["verify"]["spread_s"]}
                        for name in ("hash", "verify"):
                            mid = sorted(range(args.reps), key=lambda i: times[name][i])[args.reps // 2]
                            k[name]["last_verify_of_median"] = rounded(traces[name][mid])
                        rec[kind] = k
                        print(json.dumps({"piece_length": pl, "kind": kind, **{x: k[x] for x in (
                            "hash_over_verify", "hashlib_pool_over_hash", "hash_slower_than_verify_spread")},
                            "hash_GiB_per_s": k["hash"]["GiB_per_s"], "verify_GiB_per_s": k["verify"]["GiB_per_s"]}),
                            flush=True)
                result["piece_lengths"].append(rec)
        os.close(fd)

        # trees alone: one layer of 4 M rows, and 100,000 small layers
        import numpy as np

        rng = random.Random(0xB0)
        shapes = {"one_layer_4M_rows": [4 << 20], "100000_layers_of_1_to_64_rows": [rng.randint(1, 64)
                                                                                  for _ in range(100000)]}
        with HashPool(1 << 20) as pool:
            for name, counts in shapes.items():
                blob = np.random.default_rng(len(counts)).integers(0, 256, 32 * sum(counts), dtype=np.uint8).tobytes()
                layers, at = [], 0
                for c in counts:
                    layers.append(blob[32 * at:32 * (at + c)])
                    at += c
                t0 = time.perf_counter()
                want = [merkle.build_tree(x, 6) for x in layers]
                model_s = time.perf_counter() - t0
                trees, _ = pool.build_piece_trees(layers, 1 << 20)  # warm-up, checked (height 6)
                if trees != want:
                    raise SystemExit(f"{name}: build_piece_trees differs from merkle.build_tree")
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    pool.build_piece_trees(layers, 1 << 20)
                    ts.append(time.perf_counter() - t0)
                # the engine's call alone, on buffers made once: the upload, the passes and the download
                import ctypes

                tree_rows = sum(merkle.tree_rows(c) for c in counts)
                carr = (ctypes.c_uint32 * len(counts))(*counts)
                c_in = ctypes.create_string_buffer(blob, len(blob))
                c_tree = ctypes.create_string_buffer(32 * tree_rows)
                c_roots = ctypes.create_string_buffer(32 * len(counts))
                cs = []
                for _ in range(args.reps + 1):
                    t0 = time.perf_counter()
                    rc = pool.lib.vx_merkle_build_trees(pool._h, c_in, carr, len(counts), 6, c_tree, c_roots)
                    cs.append(time.perf_counter() - t0)
                    if rc or c_tree.raw != b"".join(want):
                        raise SystemExit(f"{name}: vx_merkle_build_trees failed or differs")
                rec = {"shape": name, "layers": len(counts), "rows": sum(counts), "tree_rows": tree_rows,
                       "build_piece_trees": summary(ts), "vx_merkle_build_trees": summary(cs[1:]),
                       "merkle_build_tree_one_thread_s": round(model_s, 3)}
                rec["build_tree_over_vx_merkle_build_trees"] = round(
                    model_s / rec["vx_merkle_build_trees"]["median_s"], 1)
                rec["build_tree_over_build_piece_trees"] = round(model_s / rec["build_piece_trees"]["median_s"], 1)
                result["trees"].append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
