#!/usr/bin/env python3
"""The v2 download path measured beside the v1 one:
runs tools/native/merkle_async_probe once per leg, each run a process of its
own under its own time limit, and writes the legs and the two conditions to
profiles/merkle/async.json.

  burst  2 GiB of registered pieces at 256 KiB and 4 MiB, GiB/s, v1 and v2
         alternating in one process
  loop   batches of 32 pieces at 32 KiB, 256 KiB and 2 MiB, p50 / p99 from a
         piece's submit to the poll that returns it

Conditions (set before measuring): on 32 x 2 MiB v2's p50 is at most half of
v1's (median of the alternating legs); in the 4 MiB burst v2's rate is at
least v1's.  Exit 1 if either fails or a leg did not finish.

--ab-lib DIR: the loop legs once more with the libvortex_amd.so in DIR, a
build with -DVX_MERKLE_ASYNC_FUSED=0 (include/vx_tuning.h: the async path on
the leaf + node kernels), recorded as "leaf_node_build"; its v1 legs are the
control between the two builds.

--zc: every run gets a third kind of leg, v2 with vx_set_merkle_zero_copy on,
alternating with the other two in the same process over the same registered
buffers.  The record (profiles/merkle/async_zc.json) sets each shape's
zero-copy figure beside the gathered v2 figure of the same run; no ratio is
required, but every verdict and the trace (zero-copy slots, no fallback) are
checked.

  python tools/merkle_async_bench.py --out profiles/merkle/async.json [--ab-lib tools/ab/leaf_node]
  python tools/merkle_async_bench.py --zc --out profiles/merkle/async_zc.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "native", "merkle_async_probe")
KiB, MiB = 1024, 1 << 20
# (mode, piece_len, further arguments, time limit in seconds)
LEGS = (("burst", 256 * KiB, [str(2 << 30)], 120), ("burst", 4 * MiB, [str(2 << 30)], 120),
        ("loop", 32 * KiB, ["32", "200"], 60), ("loop", 256 * KiB, ["32", "200"], 90),
        ("loop", 2 * MiB, ["32", "60"], 150))


def run_leg(leg, reps: int, lib_dir: str | None, zc: bool = False):
    """One probe process under its time limit; its JSON line, or None."""
    mode, plen, extra, limit = leg
    cmd = [PROBE, mode, str(plen)] + extra + [str(reps)] + (["zc"] if zc else [])
    limit = limit * 3 // 2 if zc else limit  # a third kind of leg in the same process
    env = dict(os.environ)
    if lib_dir:
        env["LD_LIBRARY_PATH"] = lib_dir + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        print(f"{' '.join(cmd)}: no result within {limit} s", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr}", file=sys.stderr)
        return None
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(dict(out, build="leaf_node" if lib_dir else "default")), flush=True)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "async.json"))
    ap.add_argument("--reps", type=int, default=5, help="alternating legs of each kind per run (the conditions need >= 5)")
    ap.add_argument("--ab-lib", help="directory of a libvortex_amd.so built with -DVX_MERKLE_ASYNC_FUSED=0")
    ap.add_argument("--zc", action="store_true",
                    help="add a v2 leg with vx_set_merkle_zero_copy on to every run (write it to "
                         "profiles/merkle/async_zc.json): no ratio is required of it, its verdicts and trace are")
    args = ap.parse_args()
    if not os.path.exists(PROBE):
        raise SystemExit(f"{PROBE} is missing: make -C tools/native")
    legs, ab_legs, ok = [], [], True
    todo = [(leg, None) for leg in LEGS]
    if args.ab_lib:
        todo += [(leg, os.path.abspath(args.ab_lib)) for leg in LEGS if leg[0] == "loop"]
    for leg, lib_dir in todo:
        out = run_leg(leg, args.reps, lib_dir, args.zc and not lib_dir)
        if out is None:
            ok = False
            break  # nothing more is started on a device that may be stuck
        (ab_legs if lib_dir else legs).append(out)

    def find(mode, plen):
        return next((x for x in legs if x["mode"] == mode and x["piece_len"] == plen), None)

    cond = {}
    lp, bu = find("loop", 2 * MiB), find("burst", 4 * MiB)
    if lp:
        cond["loop_2MiB_v2_p50_at_most_half_of_v1"] = {
            "v1_p50_ms": lp["v1_p50_ms_median"], "v2_p50_ms": lp["v2_p50_ms_median"], "ratio": lp["v2_over_v1_p50"],
            "max_ratio": 0.5, "reps": lp["reps"], "met": lp["reps"] >= 5 and lp["v2_over_v1_p50"] <= 0.5}
    if bu:
        cond["burst_4MiB_v2_at_least_v1"] = {
            "v1_GiBps": bu["v1_GiBps_median"], "v2_GiBps": bu["v2_GiBps_median"], "ratio": bu["v2_over_v1"],
            "min_ratio": 1.0, "met": bu["v2_over_v1"] >= 1.0}
    if args.zc:
        # The yardstick is the gathered v2 leg of the same run; nothing is required of the ratio.  What is
        # required: every leg finished, every verdict was right, and every zero-copy slot was one (no fallback).
        zero_copy = []
        for x in legs:
            unit = "GiBps" if x["mode"] == "burst" else "p50_ms"
            zero_copy.append({"mode": x["mode"], "piece_len": x["piece_len"], "unit": unit,
                              "v1": x[f"v1_{unit}_median"], "v2_gathered": x[f"v2_{unit}_median"],
                              "v2_zero_copy": x[f"v2zc_{unit}_median"],
                              "zero_copy_over_gathered": x["v2zc_over_v2" if x["mode"] == "burst" else "v2zc_over_v2_p50"],
                              **({} if x["mode"] == "burst" else {"v2_gathered_p99_ms": x["v2_p99_ms_median"],
                                                                  "v2_zero_copy_p99_ms": x["v2zc_p99_ms_median"]}),
                              "checked": x["wrong_verdicts"] == 0 and x["zc_trace"]["slots"] > 0
                              and x["zc_trace"]["fallback_slots"] == 0})
        ok = ok and len(legs) == len(LEGS) and all(z["checked"] for z in zero_copy)
        result = {"tool": "tools/merkle_async_bench.py --zc", "legs": legs, "zero_copy": zero_copy,
                  "conditions": cond, "ok": ok}
    else:
        ok = ok and len(cond) == 2 and all(c["met"] for c in cond.values())
        result = {"tool": "tools/merkle_async_bench.py", "legs": legs, "conditions": cond, "ok": ok}
    if args.ab_lib:
        result["leaf_node_build"] = {"define": "VX_MERKLE_ASYNC_FUSED=0", "legs": ab_legs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
