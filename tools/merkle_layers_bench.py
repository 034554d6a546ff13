#!/usr/bin/env python3
"""Many `piece layers` in one call, measured beside the only way there was
before: device.merkle_layers against a loop of
device.merkle_root per layer, on the same device buffer in one process, the
legs alternating.  Writes profiles/merkle/layers.json.

  many   100,000 layers of 2 to 64 hashes (a torrent of 10^5 multi-piece
         files): the loop makes one launch per layer, the batch one in all.
         The ratio is recorded, no figure is promised.
  one    one layer of 4,194,304 hashes (1 TiB at 256 KiB pieces): both do the
         same tile work in the same three passes, so the batch should lie
         inside the spread of the loop's own alternating runs
         ("inside_loop_spread").

A third leg, `execute`, is vx_merkle_device_layers alone on a plan made and
uploaded once: the device's share of the batch, without the host's planning
and the upload of the tiles that device.merkle_layers does per call.

A leg is timed over at least --min-s seconds of device time (device events
around the whole leg, after a warm-up of the same leg; the host clock to the
closing synchronise is recorded beside it).  Both legs' roots are compared
with each other in every shape, and those of `many` with hashlib, whose
single-thread time over the same layers is the context figure.

  python tools/merkle_layers_bench.py --out profiles/merkle/layers.json
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(torch, fn, min_s: float):
    """fn() repeated over at least min_s of device time: (ms per call by device
    events, ms per call by the host clock, calls)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # the warm-up, and the estimate of one call
    torch.cuda.synchronize()
    calls = max(1, math.ceil(min_s / max(time.perf_counter() - t0, 1e-6)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        t0 = time.perf_counter()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        dev_ms = e0.elapsed_time(e1)
        if dev_ms >= min_s * 1e3:
            return dev_ms / calls, wall_ms / calls, calls
        calls = math.ceil(calls * min_s * 1e3 / max(dev_ms, 1e-3) * 1.2)  # the estimate was short: once more, longer


def hashlib_roots(blob: bytes, counts, height: int):
    """The BEP 52 model, single thread: (roots, seconds)."""
    from vortex_amd import merkle

    pads = [merkle.pad_hash(height + k) for k in range(40)]
    sha = hashlib.sha256
    t0 = time.perf_counter()
    roots, at = [], 0
    for c in counts:
        level = [blob[32 * k:32 * k + 32] for k in range(at, at + c)]
        at += c
        k = 0
        while len(level) > 1 or (1 << k) < c:
            if len(level) & 1:
                level.append(pads[k])
            level = [sha(level[j] + level[j + 1]).digest() for j in range(0, len(level), 2)]
            k += 1
        roots.append(level[0])
    return roots, time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "layers.json"))
    ap.add_argument("--reps", type=int, default=5, help="alternating runs of each leg per shape")
    ap.add_argument("--min-s", type=float, default=0.3, help="device time of one timed leg at least")
    ap.add_argument("--layers", type=int, default=100000, help="layers of the `many` shape")
    ap.add_argument("--rows", type=int, default=4194304, help="hashes of the `one` shape")
    args = ap.parse_args()

    import torch

    from vortex_amd import _lib
    from vortex_amd import device as vdev

    if not torch.cuda.is_available():
        raise SystemExit("merkle_layers_bench needs a GPU: there is no other way to take these times")
    dev = torch.device("cuda:0")
    height = 4  # 256 KiB pieces
    rng = random.Random(0x1A7E25)
    shapes = {"many": [rng.randint(2, 64) for _ in range(args.layers)], "one": [args.rows]}
    result = {"tool": "tools/merkle_layers_bench.py", "device": torch.cuda.get_device_name(dev), "height": height,
              "min_s": args.min_s, "reps": args.reps, "shapes": {}}
    ok = True
    for name, counts in shapes.items():
        rows = sum(counts)
        gen = torch.Generator(device=dev)
        gen.manual_seed(rows)
        hashes = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        layers = [hashes[starts[f]:starts[f + 1]] for f in range(len(counts))]
        roots_batch = torch.empty((len(counts), 32), dtype=torch.uint8, device=dev)

        def batch():
            vdev.merkle_layers(hashes, counts, height, roots=roots_batch)

        # the device's share alone: planned and uploaded once, vx_merkle_device_layers per call
        plan = _lib.vx_merkle_layers_plan()
        carr = (ctypes.c_uint32 * len(counts))(*counts)
        _lib.check(_lib.lib().vx_merkle_layers_plan(carr, len(counts), ctypes.byref(plan), None, 0), "plan")
        tiles = (_lib.vx_merkle_tile * plan.n_tiles)()
        _lib.check(_lib.lib().vx_merkle_layers_plan(carr, len(counts), ctypes.byref(plan), tiles, plan.n_tiles), "plan")
        d_tiles = torch.frombuffer(tiles, dtype=torch.uint8).to(dev)
        work = torch.empty((max(plan.work_rows, 1), 32), dtype=torch.uint8, device=dev)
        roots_exec = torch.empty((len(counts), 32), dtype=torch.uint8, device=dev)

        def execute():
            _lib.check(_lib.lib().vx_merkle_device_layers(
                hashes.data_ptr(), ctypes.byref(plan), d_tiles.data_ptr(), height, work.data_ptr(),
                roots_exec.data_ptr(), None, None, int(torch.cuda.current_stream(dev).cuda_stream)), "layers")

        last = []

        def loop():
            last[:] = [vdev.merkle_root(x, height) for x in layers]

        # the two must agree before either is timed
        batch()
        execute()
        loop()
        torch.cuda.synchronize()
        same = bool(torch.equal(roots_batch, torch.stack(last))) and bool(torch.equal(roots_batch, roots_exec))
        rec = {"layers": len(counts), "rows": rows, "launches_loop": sum(max(1, math.ceil(max(c - 1, 1).bit_length() / 9))
                                                                         for c in counts),
               "launches_batch": max(math.ceil(max(c - 1, 1).bit_length() / 9) for c in counts),
               "roots_equal": same, "loop": [], "batch": [], "execute": []}
        ok = ok and same
        if name == "many":
            blob = hashes.cpu().numpy().tobytes()
            want, secs = hashlib_roots(blob, counts, height)
            rec["hashlib_single_thread_s"] = round(secs, 3)
            rec["roots_equal_hashlib"] = roots_batch.cpu().numpy().tobytes() == b"".join(want)
            ok = ok and rec["roots_equal_hashlib"]
        for _ in range(args.reps):  # alternating
            for leg, fn in (("loop", loop), ("batch", batch), ("execute", execute)):
                dev_ms, wall_ms, calls = timed(torch, fn, args.min_s)
                rec[leg].append({"device_ms": round(dev_ms, 4), "wall_ms": round(wall_ms, 4), "calls": calls})
                print(json.dumps({"shape": name, "leg": leg, **rec[leg][-1]}), flush=True)
        lo = [x["device_ms"] for x in rec["loop"]]
        ba = [x["device_ms"] for x in rec["batch"]]
        rec["loop_ms_median"], rec["batch_ms_median"] = statistics.median(lo), statistics.median(ba)
        rec["loop_ms_min_max"] = [min(lo), max(lo)]
        rec["batch_ms_min_max"] = [min(ba), max(ba)]
        ex = [x["device_ms"] for x in rec["execute"]]
        rec["execute_ms_median"], rec["execute_ms_min_max"] = statistics.median(ex), [min(ex), max(ex)]
        rec["loop_over_batch"] = round(rec["loop_ms_median"] / rec["batch_ms_median"], 2)
        if name == "one":
            rec["inside_loop_spread"] = min(lo) <= rec["batch_ms_median"] <= max(lo)
            rec["execute_inside_loop_spread"] = min(lo) <= rec["execute_ms_median"] <= max(lo)
        result["shapes"][name] = rec
        del layers, hashes
    result["ok"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v if k != "shapes" else {s: {q: r[q] for q in r if q not in ("loop", "batch", "execute")}
                                                    for s, r in v.items()}) for k, v in result.items()}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
