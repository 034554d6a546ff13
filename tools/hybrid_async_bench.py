#!/usr/bin/env python3
"""A hybrid torrent's download path, vx_hybrid_submit (leg A) beside the
two-submit way it replaces (leg B: vx_submit over a padded copy plus
vx_merkle_submit) and vx_merkle_submit alone (leg V): runs
tools/native/hybrid_async_probe once per row, each run a process of its own
under its own time limit, and writes the rows and the conditions to
profiles/hybrid/async.json.

  burst  2 GiB of registered 256 KiB pieces, GiB/s of piece bytes, the legs
         alternating in one process, median of 5 with the range
  loop   batches of 32 pieces at 32 KiB, 256 KiB and 2 MiB, p50 from a piece's
         (first) submit to the poll that completes it

Conditions (set before measuring):
  burst   A >= 1.5 x B: leg B moves every byte over PCIe twice, so the model
          says 2 x; the slack is the gathered slot's SHA-1 starting after its
          transfer and not during it.
  loop    at 256 KiB and 2 MiB, A's median <= 1.05 x B's median + B's own range
          over its five legs: leg B's v1 kernel reads host memory itself and so
          hides the transfer that A's chain has to wait for, 32 pieces'
          transfer over one piece's chain, 1 + (32 x 64 B) / (0.76 us x 50
          GiB/s) = 1.05.
  32 KiB  no bound: launches and small copies bind it; A, B and V side by side.
Every row runs once more with no padded piece (pad_every 0), recorded as
"unpadded_control": what of A - B belongs to the padded pieces' zero blocks.
Exit 1 if a condition fails or a row did not finish.

  python tools/hybrid_async_bench.py --out profiles/hybrid/async.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "native", "hybrid_async_probe")
KiB, MiB = 1024, 1 << 20
# (mode, piece_len, further arguments, time limit in seconds, pad_every); pad_every 16: every 16th piece ends
# a file (3/4 data, 1/4 pad), the rows of the conditions; 0: no piece is padded, the control rows
ROWS = (("burst", 256 * KiB, [str(2 << 30)], 150, 16), ("loop", 32 * KiB, ["32", "200"], 60, 16),
        ("loop", 256 * KiB, ["32", "200"], 120, 16), ("loop", 2 * MiB, ["32", "40"], 180, 16),
        ("burst", 256 * KiB, [str(2 << 30)], 150, 0), ("loop", 32 * KiB, ["32", "200"], 60, 0),
        ("loop", 256 * KiB, ["32", "200"], 120, 0), ("loop", 2 * MiB, ["32", "40"], 180, 0))


def run_row(row, reps: int):
    """One probe process under its time limit; its JSON line, or None."""
    mode, plen, extra, limit, pad_every = row
    cmd = [PROBE, mode, str(plen)] + extra + [str(reps), str(pad_every)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"{' '.join(cmd)}: no result within {limit} s", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr}", file=sys.stderr)
        return None
    out = dict(json.loads(r.stdout.strip().splitlines()[-1]), pad_every=pad_every)
    print(json.dumps(out), flush=True)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid", "async.json"))
    ap.add_argument("--reps", type=int, default=5, help="alternating legs of each kind per row (the conditions need >= 5)")
    args = ap.parse_args()
    if not os.path.exists(PROBE):
        raise SystemExit(f"{PROBE} is missing: make -C tools/native")
    rows, ok = [], True
    for row in ROWS:
        out = run_row(row, args.reps)
        if out is None:
            ok = False
            break  # nothing more is started on a device that may be stuck
        rows.append(out)

    def find(mode, plen, pad_every=16):
        return next((x for x in rows if x["mode"] == mode and x["piece_len"] == plen and x["pad_every"] == pad_every),
                    None)

    cond = {}
    bu = find("burst", 256 * KiB)
    if bu:
        cond["burst_256KiB_A_at_least_1.5x_B"] = {
            "A_GiBps": bu["A_median"], "B_GiBps": bu["B_median"], "ratio": bu["A_over_B"], "min_ratio": 1.5,
            "reps": bu["reps"], "met": bu["reps"] >= 5 and bu["A_median"] >= 1.5 * bu["B_median"]}
    for plen, name in ((256 * KiB, "256KiB"), (2 * MiB, "2MiB")):
        lp = find("loop", plen)
        if lp:
            bound = 1.05 * lp["B_median"] + lp["B_range"]
            cond[f"loop_{name}_A_p50_within_1.05x_B_plus_range"] = {
                "A_p50_ms": lp["A_median"], "B_p50_ms": lp["B_median"], "B_range_ms": lp["B_range"],
                "bound_ms": round(bound, 3), "reps": lp["reps"], "met": lp["reps"] >= 5 and lp["A_median"] <= bound}
    small = find("loop", 32 * KiB)
    side_by_side = None
    if small:
        side_by_side = {"A_p50_ms": small["A_median"], "B_p50_ms": small["B_median"], "V_p50_ms": small["V_median"],
                        "A_minus_B_ms": round(small["A_median"] - small["B_median"], 3)}
    # the same rows with no padded piece: what of A - B is the padded pieces' zero blocks (no condition)
    control = {}
    for mode, plen, name in (("burst", 256 * KiB, "burst_256KiB"), ("loop", 32 * KiB, "loop_32KiB"),
                             ("loop", 256 * KiB, "loop_256KiB"), ("loop", 2 * MiB, "loop_2MiB")):
        c = find(mode, plen, 0)
        if c:
            control[name] = {"A": c["A_median"], "B": c["B_median"], "V": c["V_median"], "A_over_B": c["A_over_B"],
                             "unit": c["unit"]}
    ok = ok and len(cond) == 3 and all(c["met"] for c in cond.values())
    result = {"tool": "tools/hybrid_async_bench.py", "rows": rows, "conditions": cond,
              "loop_32KiB_no_bound": side_by_side, "unpadded_control": control, "ok": ok}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
