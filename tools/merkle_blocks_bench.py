#!/usr/bin/env python3
"""The block check beside the leaf + node pair it shares its lanes with
("Block checks"): device.merkle_block_check against
device.merkle_ragged on the same HBM buffer in one process, the legs
alternating.  Writes profiles/merkle/block_check.json.

  4,096 x 4 MiB      256 leaf slots per piece: four bitmap words
  65,536 x 256 KiB   16 leaf slots per piece: one bitmap word, 4 pieces a wave

Legs, --reps timed runs of each, alternating:

  merkle_ragged   the leaf kernel (writes every leaf row) and the node launch
  check           merkle_block_check, bitmap only: the leaf kernel's hashing,
                  one expected row loaded per lane, a ballot per wave
  check_leaves    the same with leaves_out: it also writes every leaf row

The expected rows are merkle_ragged's own leaves with every 97th row off by a
bit, so the bitmap is known; both forms' bitmaps and the leaves are compared
before anything is timed.  A step is one call over the whole buffer, timed in
device time (events around each step) between the shader clock stamps bench.py
uses.  The ratio merkle_ragged / check of the median step times is recorded;
no figure is promised.

  python tools/merkle_blocks_bench.py --out profiles/merkle/block_check.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK = 16384
SHAPES = ((4096, 4 << 20), (65536, 256 * 1024))
EVERY = 97  # rows apart of the expected rows that are off


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "block_check.json"))
    ap.add_argument("--reps", type=int, default=3, help="alternating timed runs of each leg per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=400.0, help="timed window per leg")
    ap.add_argument("--scale", type=int, default=1, help="divide the piece counts by this (a rehearsal)")
    args = ap.parse_args()

    import torch

    from merkle_bench import timed
    from vortex_amd import device as vdev
    from vortex_amd import merkle

    if not torch.cuda.is_available():
        raise SystemExit("merkle_blocks_bench needs a GPU: a rate is a measurement on the device")
    dev = torch.device("cuda:0")
    result = {"tool": "tools/merkle_blocks_bench.py", "device": torch.cuda.get_device_properties(dev).name,
              "reps": args.reps, "target_ms": args.target_ms, "bad_row_every": EVERY, "shapes": []}
    for n, plen in SHAPES:
        n = max(1, n // args.scale)
        lw = merkle.log2_width(plen)
        rows, nbytes = n << lw, n * plen
        data = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        vdev.synth_fill(data, n, plen, seed=0xB10C + lw)
        offs = torch.arange(n, dtype=torch.int64, device=dev) * plen
        lens = torch.full((n,), plen, dtype=torch.int32, device=dev)
        leaves = torch.empty((rows, 32), dtype=torch.uint8, device=dev)
        roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        vdev.merkle_ragged(data, offs, lens, lw, leaves=leaves, roots=roots)  # validates the layout once
        expected = leaves.clone()
        expected[::EVERY, 31] ^= 1
        words = merkle.bitmap_words(n, lw)
        bad = torch.full((words,), -1, dtype=torch.int64, device=dev)
        bad2 = torch.full((words,), -1, dtype=torch.int64, device=dev)
        leaves2 = torch.full((rows, 32), 0xFF, dtype=torch.uint8, device=dev)

        def pair():
            vdev.merkle_ragged(data, offs, lens, lw, leaves=leaves, roots=roots, validate=False)

        def check():
            vdev.merkle_block_check(data, offs, lens, lw, expected_leaves=expected, bad=bad, want_leaves=False,
                                    validate=False)

        def check_leaves():
            vdev.merkle_block_check(data, offs, lens, lw, expected_leaves=expected, bad=bad2, leaves=leaves2,
                                    validate=False)

        check()
        check_leaves()
        torch.cuda.synchronize(dev)
        # what is timed computes the right thing: bit g of the bitmap is set iff g % EVERY == 0
        g = torch.arange(rows, dtype=torch.int64, device=dev)
        if lw >= 6:
            word, bit = g >> 6, g & 63
        else:
            word, bit = g >> lw, g & ((1 << lw) - 1)
        want = torch.zeros(words, dtype=torch.int64, device=dev)
        hit = (g % EVERY) == 0
        want.scatter_add_(0, word[hit], torch.ones_like(g[hit]) << bit[hit])  # (bits are distinct: add is or)
        same = bool(torch.equal(bad, want)) and bool(torch.equal(bad2, want)) and bool(torch.equal(leaves2, leaves))
        if not same:
            raise SystemExit(f"{n} x {plen}: the block check differs from merkle_ragged's leaves")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pair()
        e1.record()
        torch.cuda.synchronize(dev)
        steps = max(5, min(200, int(args.target_ms / max(e0.elapsed_time(e1), 1e-3))))
        runs = {"merkle_ragged": [], "check": [], "check_leaves": []}
        for _ in range(args.reps):  # alternating
            for name, fn in (("merkle_ragged", pair), ("check", check), ("check_leaves", check_leaves)):
                t, clock = timed(fn, args.warmup, steps, dev)
                rec = {k: round(v, 4) if isinstance(v, float) else v for k, v in t.items()}
                rec.update(GiB_per_s=round(nbytes / (t["step_ms_median"] * 1e-3) / 2 ** 30, 1),
                           clock_GHz=clock.get("GHz_mean"), clock_GHz_min=clock.get("GHz_min"))
                runs[name].append(rec)
                print(json.dumps({"pieces": n, "piece_len": plen, "leg": name, **rec}), flush=True)
        med = {k: statistics.median(r["step_ms_median"] for r in v) for k, v in runs.items()}
        lo = [r["step_ms_median"] for r in runs["merkle_ragged"]]
        shape = {"pieces": n, "piece_len": plen, "bytes": nbytes, "log2_width": lw, "bitmap_words": words,
                 "bitmap_equal": same, "runs": runs, "step_ms_median": {k: round(v, 4) for k, v in med.items()},
                 "merkle_ragged_ms_min_max": [min(lo), max(lo)],
                 "ragged_over_check": round(med["merkle_ragged"] / med["check"], 3),
                 "ragged_over_check_leaves": round(med["merkle_ragged"] / med["check_leaves"], 3)}
        result["shapes"].append(shape)
        del data, leaves, leaves2, expected, bad, bad2, want, g, word, bit, hit
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"shapes": [{k: v for k, v in s.items() if k != "runs"} for s in result["shapes"]]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
