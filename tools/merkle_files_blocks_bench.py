#!/usr/bin/env python3
"""What checking and keeping the 16 KiB leaf layer costs the v2 files calls
(DESIGN.md §3.7 "Block checks from disk").

One file of BASELINE config 5's size (2,907,832,320 bytes), page cache warm, at
piece lengths 256 KiB, 4 MiB and 16 MiB.  One byte is flipped in every 100th
piece (1 % of the pieces, a block chosen by the piece's number); the expected
tables are hashlib's over the undamaged file.  Five legs alternate within this
one process:

  (a) plain        HashPool.verify_merkle_files: the call this feature leaves as
                   it was
  (b) blocks       HashPool.verify_merkle_files_blocks: the same pass, plus the
                   bad-block bitmap and layer_ok
  (c) hash         HashPool.hash_merkle_files
  (d) hash_leaves  HashPool.hash_merkle_files_leaves: the same pass, plus the
                   leaf table
  (e) two_pass     what (b) replaces: verify_merkle_files, then the failed
                   pieces read again (pread) and pushed through
                   HashPool.check_blocks with their stored leaf rows

Before anything is timed the verdicts, bitmaps and tables of every leg are
checked against the model.  A call is timed with the host clock around it;
medians, minima and maxima of --reps calls per leg are recorded with the
blocks / plain and hash_leaves / hash ratios, (a)'s and (b)'s last_verify() of
their median calls, and whether (b) is slower than (a) by more than (a)'s own
spread (max - min) across its runs.  No ratio is a condition: the tool fails
only on a wrong result.

  python tools/merkle_files_blocks_bench.py --out profiles/merkle/files_blocks.json
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
LEGS = ("plain", "blocks", "hash", "hash_leaves", "two_pass")


def write_file(path: str, total: int) -> None:
    import numpy as np

    rng = np.random.default_rng(0x5EED0B10)
    with open(path, "wb") as f:
        left = total
        while left:
            n = min(left, 64 << 20)
            f.write(rng.bytes(n))
            left -= n
        f.flush()
        os.fsync(f.fileno())  # writeback done before anything is timed


def leaf_table(ex: ThreadPoolExecutor, fd: int, total: int) -> bytes:
    """hashlib over every 16 KiB block, 4 MiB per task (also warms the page cache)."""
    span = 4 << 20

    def part(off):
        data = os.pread(fd, min(span, total - off), off)
        return b"".join(hashlib.sha256(data[o:o + BLOCK]).digest() for o in range(0, len(data), BLOCK))

    return b"".join(ex.map(part, range(0, total, span)))


def piece_root(rows: bytes, log2w: int) -> bytes:
    level = [rows[k:k + 32] for k in range(0, len(rows), 32)]
    level += [bytes(32)] * ((1 << log2w) - len(level))
    while len(level) > 1:
        level = [hashlib.sha256(level[k] + level[k + 1]).digest() for k in range(0, len(level), 2)]
    return level[0]


def flip(fd: int, at: int) -> None:
    b = os.pread(fd, 1, at)
    os.pwrite(fd, bytes([b[0] ^ 0x40]), at)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "files_blocks.json"))
    ap.add_argument("--reps", type=int, default=5, help="timed calls per leg and piece length (at least 3)")
    ap.add_argument("--scale", type=float, default=1.0, help="< 1 shrinks the file (rehearsal; the record says so)")
    ap.add_argument("--dir", help="where the file goes (default: bench.py's choice, a disk-backed directory)")
    args = ap.parse_args()
    if args.reps < 3:
        raise SystemExit("--reps must be at least 3")

    import torch

    from bench import fs_type, reverify_dir
    from vortex_amd import merkle
    from vortex_amd.hash_pool import HashPool

    if not torch.cuda.is_available():
        raise SystemExit("merkle_files_blocks_bench needs a GPU: a rate is a measurement on the device")
    total = TOTAL if args.scale >= 1.0 else max(BLOCK, int(TOTAL * args.scale) // BLOCK * BLOCK)
    d = args.dir or reverify_dir()
    path = os.path.join(d, f"vx_files_blocks_{os.getpid()}.bin")
    result = {"tool": "tools/merkle_files_blocks_bench.py", "device": torch.cuda.get_device_properties(0).name,
              "file_bytes": total, "scale": args.scale, "fs": fs_type(d), "reps": args.reps,
              "damage": "one byte flipped in every 100th piece",
              "timing": "host clock around each synchronous call, page cache warm, legs alternating "
                        + ", ".join(LEGS) + " within each repetition", "piece_lengths": []}
    try:
        t0 = time.perf_counter()
        write_file(path, total)
        result["write_s"] = round(time.perf_counter() - t0, 2)
        fd = os.open(path, os.O_RDWR)
        with ThreadPoolExecutor(CPU_THREADS) as ex:
            table = leaf_table(ex, fd, total)
            for pl in PIECE_LENGTHS:
                lens, log2w = merkle.file_pieces(total, pl)
                n, W = len(lens), pl // BLOCK
                first, blocks, leaf_rows = merkle.leaf_layout([total], pl)
                assert 32 * leaf_rows == len(table)
                rows_of = lambda i: table[32 * first[i]:32 * (first[i] + blocks[i])]  # noqa: E731
                roots = b"".join(ex.map(lambda i: piece_root(rows_of(i), log2w[i]), range(n)))
                damaged = {i: (7 * i) % blocks[i] for i in range(50 % n, n, 100)}
                for i, b in damaged.items():
                    flip(fd, i * pl + b * BLOCK + 5)
                wpp = max(1, W // 64)
                want_words = [0] * (n * wpp)
                for i, b in damaged.items():
                    want_words[i * wpp + (b >> 6)] |= 1 << (b & 63)
                want_matched = [i not in damaged for i in range(n)]
                with HashPool(pl, slots=4, slot_bytes=512 << 20, batch_pieces=4096) as pool:
                    def plain():
                        return pool.verify_merkle_files([path], [total], pl, roots, io_threads=16)

                    def with_blocks():
                        return pool.verify_merkle_files_blocks([path], [total], pl, roots, table, io_threads=16)

                    def hashed():
                        return pool.hash_merkle_files([path], [total], pl, io_threads=16)

                    def hashed_leaves():
                        return pool.hash_merkle_files_leaves([path], [total], pl, io_threads=16)

                    def two_pass():
                        got, _ = pool.verify_merkle_files([path], [total], pl, roots, io_threads=16)
                        failed = [i for i, v in enumerate(got) if not v]
                        pieces = [os.pread(fd, lens[i], i * pl) for i in failed]
                        stored = [rows_of(i) + bytes(32 * (W - blocks[i])) for i in failed]
                        bad, _ = pool.check_blocks(pieces, pl, stored) if failed else ([], None)
                        return dict(zip(failed, bad))

                    # every leg's result, before anything is timed
                    got, errs = plain()
                    if (got, errs) != (want_matched, 0):
                        raise SystemExit(f"plain at {pl}: verdicts differ from the model")
                    res = with_blocks()
                    if (res.matched, res.layer_ok, res.bad, res.io_errors) != (want_matched, [True] * n, want_words, 0):
                        raise SystemExit(f"blocks at {pl}: verdicts, layer_ok or bitmap differ from the model")
                    if res.bad_counts != [int(i in damaged) for i in range(n)]:
                        raise SystemExit(f"blocks at {pl}: bad counts differ from the model")
                    h_rows, h_ok, h_tree, h_errs = hashed()
                    l_rows, l_ok, l_tree, l_errs, leaves = hashed_leaves()
                    if (h_rows, h_ok, h_tree, h_errs) != (l_rows, l_ok, l_tree, l_errs) or not all(h_ok):
                        raise SystemExit(f"hash_leaves at {pl}: rows or trees differ from hash_merkle_files'")
                    differ = [r for r in range(leaf_rows) if leaves[32 * r:32 * r + 32] != table[32 * r:32 * r + 32]]
                    if differ != sorted(first[i] + b for i, b in damaged.items()):
                        raise SystemExit(f"hash_leaves at {pl}: the leaf table differs from hashlib's")
                    if two_pass() != {i: [b] for i, b in damaged.items()}:
                        raise SystemExit(f"two_pass at {pl}: bad blocks differ from the model")

                    legs = dict(zip(LEGS, (plain, with_blocks, hashed, hashed_leaves, two_pass)))
                    times = {name: [] for name in LEGS}
                    traces = {"plain": [], "blocks": []}
                    for _ in range(args.reps):
                        for name, leg in legs.items():
                            t0 = time.perf_counter()
                            leg()
                            times[name].append(time.perf_counter() - t0)
                            if name in traces:
                                traces[name].append(pool.last_verify())
                for i, b in damaged.items():  # the file as it was, for the next piece length
                    flip(fd, i * pl + b * BLOCK + 5)
                rec = {"piece_length": pl, "pieces": n, "damaged_pieces": len(damaged)}
                for name, ts in times.items():
                    med = statistics.median(ts)
                    rec[name] = {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                                 "GiB_per_s": round(total / GIB / med, 2), "calls_s": [round(t, 5) for t in ts]}
                    if name in traces:
                        k = sorted(range(len(ts)), key=lambda i: ts[i])[len(ts) // 2]
                        rec[name]["last_verify_of_median"] = {
                            key: (round(v, 3) if isinstance(v, float) else v) for key, v in traces[name][k].items()}
                a, b = rec["plain"], rec["blocks"]
                rec["blocks_over_plain"] = round(b["median_s"] / a["median_s"], 4)
                rec["hash_leaves_over_hash"] = round(rec["hash_leaves"]["median_s"] / rec["hash"]["median_s"], 4)
                rec["two_pass_over_blocks"] = round(rec["two_pass"]["median_s"] / b["median_s"], 4)
                rec["plain_spread_s"] = round(a["max_s"] - a["min_s"], 5)
                rec["blocks_slower_than_plain_spread"] = b["median_s"] - a["median_s"] > a["max_s"] - a["min_s"]
                result["piece_lengths"].append(rec)
                print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "calls_s"} if isinstance(v, dict) else v)
                                  for k, v in rec.items()}), flush=True)
        os.close(fd)
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
