#!/usr/bin/env python3
"""Device time of the zero-tail kernel against the only way the
parent tree could hash a hybrid piece's pad: the chunked split kernel continuing
the same chaining states through a device buffer of zeros.

Shapes: 65,536 lanes x Z = 4,095 zero blocks (a 256 KiB piece that is one data
block and pad) and 1,024 lanes x Z = 65,535 (a 4 MiB one).  Every lane owns 64
bytes of data; the chunked kernel hashes them once and leaves the states both
legs start from.

  (a) zero_tail   sha1_zero_tail_kernel from the states: nothing is read
  (b) chunk_zeros the chunked split kernel over pad_len zero bytes per lane in
                  HBM (each lane its own, as materialised pads would lie;
                  --shared-zeros: all lanes read one pad, served from cache),
                  final chunk, so it pads and emits as (a) does

The digests of both legs must be equal for every lane and equal hashlib's for
a few.  Each leg runs --reps times, alternating, in device time (events around
the launch) between the shader clock stamps bench.py uses; medians are
reported with µs per zero block (leg time / Z: the chain a wave walks, beside
§3.5's 0.76 µs per data block) and SIMD cycles per wave VALU op from the ISA
op counts (--isa recounts the zero loop's).

  python tools/hybrid_tail_bench.py --out profiles/hybrid/tail.json [--isa sha1_tail_kernels.s]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((65536, 4095), (1024, 65535))
SHA1_VALU_PER_BLOCK = 613   # sha1_device.hpp: a data block of the general compression
ZERO_VALU_PER_BLOCK = 411   # hipcc's ISA of the zero-block loop; --isa recounts it


def isa_zero_loop(path: str) -> dict:
    """VALU instructions of sha1_zero_tail_kernel's zero-block loop (its one
    inner loop: one block per trip), from hipcc's -save-temps ISA."""
    text = open(path).read()
    m = re.search(r"^(_ZN\S*sha1_zero_tail_kernel\S*):", text, re.M)
    if not m:
        raise SystemExit(f"{path}: sha1_zero_tail_kernel not found")
    body = text[m.end():]
    body = body[:body.index("s_endpgm")]
    head = re.search(r"^(\.LBB\d+_\d+):[^\n]*\n[^\n]*This Inner Loop Header: Depth=1", body, re.M)
    back = head and list(re.finditer(r"s_c?branch\w*\s+" + re.escape(head.group(1)) + r"\b", body[head.end():]))
    if not head or not back:
        raise SystemExit(f"{path}: no zero-block loop found")
    loop = body[head.start():head.end() + back[-1].end()]
    ops: dict = {}
    for op in re.findall(r"^\s+(v_[a-z0-9_]+)", loop, re.M):
        ops[op] = ops.get(op, 0) + 1
    return {"valu_per_block": sum(ops.values()), "by_op": dict(sorted(ops.items(), key=lambda kv: -kv[1])),
            "source": os.path.basename(path)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid", "tail.json"))
    ap.add_argument("--isa", help="hipcc -save-temps ISA of sha1_tail_kernels.hip: recount the zero loop's VALU ops")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--shared-zeros", action="store_true", help="leg (b): every lane reads the same pad")
    args = ap.parse_args()

    import torch

    from bench import ClockStamps
    from vortex_amd._lib import check, tuning

    if not torch.cuda.is_available():
        raise SystemExit("hybrid_tail_bench needs a GPU: a time is a measurement on the device")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    simds = props.multi_processor_count * 4
    isa = isa_zero_loop(args.isa) if args.isa else None
    zero_valu = isa["valu_per_block"] if isa else ZERO_VALU_PER_BLOCK
    T = tuning()
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    result = {"tool": "tools/hybrid_tail_bench.py", "device": props.name, "compute_units": props.multi_processor_count,
              "reps": args.reps, "zeros": "shared" if args.shared_zeros else "per lane",
              "isa": isa or {"valu_per_block": ZERO_VALU_PER_BLOCK, "source": "DESIGN.md §3.8"},
              "sha1_valu_per_block": SHA1_VALU_PER_BLOCK, "data_block_us_section_3_5": 0.76, "shapes": []}
    for idx in (int(x) for x in args.shapes.split(",")):
        n, Z = SHAPES[idx]
        pl, pad = (Z + 1) * 64, Z * 64
        gen = torch.Generator(device="cpu").manual_seed(0x7A11 + idx)
        data = torch.randint(0, 256, (n * 64,), dtype=torch.uint8, generator=gen)
        zeros_bytes = pad if args.shared_zeros else n * pad
        buf = torch.zeros(n * 64 + zeros_bytes, dtype=torch.uint8, device=dev)
        buf[:n * 64] = data.to(dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        offs0 = ar * 64
        zoffs = torch.full_like(ar, n * 64) if args.shared_zeros else n * 64 + ar * pad
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda v: torch.full((n,), v, dtype=torch.int64, device=dev)  # noqa: E731
        pids = torch.arange(n, dtype=torch.int32, device=dev)
        states = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        dig = {k: torch.zeros((n, 20), dtype=torch.uint8, device=dev) for k in ("zero_tail", "chunk_zeros")}
        len64, lpad, zero64, plen64 = i32(64), i32(pad), i64(0), i64(pl)
        poff64 = i64(64)
        # the data block of every lane, once: a non-final chunk leaves the states
        check(T.vx_tuning_chunk_kernel(buf.data_ptr(), offs0.data_ptr(), len64.data_ptr(), n, pids.data_ptr(),
                                       zero64.data_ptr(), plen64.data_ptr(), states.data_ptr(),
                                       dig["chunk_zeros"].data_ptr(), sp), "vx_tuning_chunk_kernel", T)
        torch.cuda.synchronize(dev)
        work = states.clone()  # leg (b) never stores a state (its chunk is final); kept apart all the same

        def zero_tail():
            check(T.vx_tuning_zero_tail_kernel(buf.data_ptr(), offs0.data_ptr(), len64.data_ptr(), lpad.data_ptr(), n,
                                               pl, states.data_ptr(), dig["zero_tail"].data_ptr(), sp),
                  "vx_tuning_zero_tail_kernel", T)

        def chunk_zeros():
            check(T.vx_tuning_chunk_kernel(buf.data_ptr(), zoffs.data_ptr(), lpad.data_ptr(), n, pids.data_ptr(),
                                           poff64.data_ptr(), plen64.data_ptr(), work.data_ptr(),
                                           dig["chunk_zeros"].data_ptr(), sp), "vx_tuning_chunk_kernel", T)

        legs = (("zero_tail", zero_tail), ("chunk_zeros", chunk_zeros))
        for _, fn in legs:  # warm-up, then checked
            fn()
        torch.cuda.synchronize(dev)
        if not torch.equal(dig["zero_tail"], dig["chunk_zeros"]):
            bad = (dig["zero_tail"] != dig["chunk_zeros"]).any(dim=1).sum().item()
            raise SystemExit(f"{n} x Z={Z}: {bad} digests of the zero-tail kernel differ from the chunked kernel's")
        host = dig["zero_tail"].cpu().numpy()
        for j in (0, 63, 64, n - 1):
            want = hashlib.sha1(data[j * 64:(j + 1) * 64].numpy().tobytes() + bytes(pad)).digest()
            if host[j].tobytes() != want:
                raise SystemExit(f"{n} x Z={Z}: lane {j} differs from hashlib")
        ms = {k: [] for k, _ in legs}
        clocks = {k: [] for k, _ in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                clk = ClockStamps(dev, stream)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                clk.stamp(0)
                a.record(stream)
                fn()
                b.record(stream)
                clk.stamp(1)
                torch.cuda.synchronize(dev)
                ms[name].append(a.elapsed_time(b))
                clocks[name].append(clk.result().get("GHz_mean"))
        shape = {"lanes": n, "zero_blocks": Z, "piece_length": pl, "pad_len": pad}
        for name, valu in (("zero_tail", zero_valu), ("chunk_zeros", SHA1_VALU_PER_BLOCK)):
            med = statistics.median(ms[name])
            ghz = [g for g in clocks[name] if g]
            g = statistics.median(ghz) if ghz else None
            waves = n / 64.0
            shape[name] = {
                "ms_median": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                "ms": [round(x, 4) for x in ms[name]], "us_per_block": round(med * 1e3 / Z, 4),
                "valu_per_block": valu, "clock_GHz": g,
                # (more waves than SIMDs queue; with at most one wave per SIMD this is the chain's own rate)
                "cycles_per_valu": round(med * 1e-3 * g * 1e9 * min(simds, waves) / (waves * Z * valu), 3) if g else None}
        shape["chunk_over_tail"] = round(shape["chunk_zeros"]["ms_median"] / shape["zero_tail"]["ms_median"], 3)
        shape["valu_ratio"] = round(SHA1_VALU_PER_BLOCK / zero_valu, 3)
        result["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
        del buf, dig, states, work
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
