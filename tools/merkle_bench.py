#!/usr/bin/env python3
"""Device-resident rate of the BitTorrent v2 merkle path.

For each shape the merkle kernels (leaf + node, vx_merkle_device_uniform) and
the SHA-1 kernel run on the same HBM buffer in this one process:

  65,536 x 256 KiB     merkle  vs  sha1_uniform
  1,024 x 4 MiB        merkle  vs  sha1_ragged   (one 65,537-block chain per piece)
  1,048,576 x 16 KiB   merkle  (plain SHA-256: one leaf per piece)

A step is one call over the whole buffer.  Steps are timed in device time
(events around each step, after warm-up steps) and bracketed by the shader
clock stamps bench.py uses (vx_tuning_clock_stamp), so each rate comes with
the clock it was measured at.  Per kernel the record holds GiB/s, the fraction
of the 8 TB/s HBM peak, the VALU ops per 64-byte block (counted from the
compiler's ISA with --isa, else the figures of DESIGN.md) and SIMD cycles per
wave VALU op = kernel time x clock x SIMDs / (waves x blocks x ops per block).

One condition: on 1,024 x 4 MiB the merkle path must be at least 2x the SHA-1
ragged rate measured beside it (a piece is 256 independent lanes instead of
one chain); the ratio is recorded and the tool exits 1 below it.

--blocks-leg K: on 65,536 x 256 KiB the block-stream kernel and the node entry
(merkle_blocks + merkle_nodes, the re-verify's kernels) run over the same
buffer beside merkle_uniform, K timed runs of each, alternating; both are
recorded with the spread between merkle_uniform's own runs.

--pieces-leg K: on 65,536 x 256 KiB and 1,024 x 4 MiB the fused piece kernel
(merkle_pieces, the async path's kernel) runs beside the leaf + node pair
(merkle_ragged) on the same buffer, K alternating timed runs of each, recorded
with the spread between the pair's own runs.

  python tools/merkle_bench.py --out profiles/merkle/device.json [--isa sha256_kernels.s]
  python tools/merkle_bench.py --shapes 0 --blocks-leg 3 --out profiles/merkle/blocks.json
  python tools/merkle_bench.py --shapes 0,1 --pieces-leg 3 --no-sha1 --out profiles/merkle/pieces.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BLOCK = 16384
HBM_PEAK = 8e12  # bytes/s
SHA1_VALU_PER_BLOCK = 613  # sha1_device.hpp
SHA256_VALU_PER_BLOCK = 1401  # hipcc's ISA of merkle_leaf_kernel's loop; --isa recounts it
SHAPES = ((65536, 256 * 1024, "sha1_uniform"), (1024, 4 << 20, "sha1_ragged"), (1 << 20, 16 * 1024, None))


def isa_valu_per_block(path: str) -> dict:
    """VALU instructions per 64-byte block in the streaming loop of
    merkle_leaf_kernel<false>, from hipcc's -save-temps ISA: the loop is the
    stretch between the kernel's first inner-loop header label and the last
    branch back to it, and holds two 128-byte groups = four blocks."""
    text = open(path).read()
    m = re.search(r"^(_ZN\S*merkle_leaf_kernelILb0E\S*):", text, re.M)
    if not m:
        raise SystemExit(f"{path}: merkle_leaf_kernel<false> not found")
    body = text[m.end():]
    body = body[:body.index("s_endpgm")]
    head = re.search(r"^(\.LBB\d+_\d+):[^\n]*\n[^\n]*This Inner Loop Header: Depth=1", body, re.M)
    back = head and list(re.finditer(r"s_c?branch\w*\s+" + re.escape(head.group(1)) + r"\b", body[head.end():]))
    if not head or not back:
        raise SystemExit(f"{path}: no streaming loop found in the leaf kernel")
    loop = body[head.start():head.end() + back[-1].end()]
    ops: dict = {}
    for op in re.findall(r"^\s+(v_[a-z0-9_]+)", loop, re.M):
        ops[op] = ops.get(op, 0) + 1
    total = sum(ops.values())
    return {"valu_per_block": total / 4.0, "loop_valu": total, "blocks_in_loop": 4,
            "by_op_per_block": {k: v / 4.0 for k, v in sorted(ops.items(), key=lambda kv: -kv[1])},
            "source": os.path.basename(path)}


def tree_root(data: bytes, log2_width: int) -> bytes:
    rows = [hashlib.sha256(data[o:o + BLOCK]).digest() if o < len(data) else bytes(32)
            for o in range(0, BLOCK << log2_width, BLOCK)]
    while len(rows) > 1:
        rows = [hashlib.sha256(rows[k] + rows[k + 1]).digest() for k in range(0, len(rows), 2)]
    return rows[0]


def timed(fn, warmup: int, steps: int, dev):
    """Mean device ms per step of fn() and the shader clock over the steps."""
    import torch

    from bench import ClockStamps

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    stream = torch.cuda.current_stream(dev)
    clk = ClockStamps(dev, stream)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    clk.stamp(0)
    for a, b in evs:
        a.record(stream)
        fn()
        b.record(stream)
    clk.stamp(1)
    torch.cuda.synchronize(dev)
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return {"step_ms_mean": sum(ms) / steps, "step_ms_median": ms[steps // 2], "step_ms_min": ms[0],
            "step_ms_max": ms[-1], "steps": steps, "warmup": warmup}, clk.result()


def record(t: dict, clock: dict, nbytes: int, lanes: int, blocks_per_lane: int, valu_per_block: float,
           simds: int) -> dict:
    s = t["step_ms_mean"] * 1e-3
    ghz = clock.get("GHz_mean")
    wave_ops = (lanes / 64.0) * blocks_per_lane * valu_per_block
    out = dict(t, GiB_per_s=round(nbytes / s / 2 ** 30, 1), frac_of_8TBps=round(nbytes / s / HBM_PEAK, 4),
               valu_per_block=valu_per_block, clock_GHz=ghz, clock_GHz_min=clock.get("GHz_min"))
    out["cycles_per_valu"] = round(s * ghz * 1e9 * simds / wave_ops, 3) if ghz else None
    for k in ("step_ms_mean", "step_ms_median", "step_ms_min", "step_ms_max"):
        out[k] = round(out[k], 4)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle", "device.json"))
    ap.add_argument("--isa", help="hipcc -save-temps ISA of sha256_kernels.hip: recount the VALU ops per block")
    ap.add_argument("--lib", help="load this build of libvortex_amd.so instead (A/B of build flags)")
    ap.add_argument("--label", default="default build")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=400.0, help="timed window per kernel and shape")
    ap.add_argument("--shapes", default="0,1,2", help="indices into the three shapes")
    ap.add_argument("--blocks-leg", type=int, default=0, metavar="K",
                    help="on 65,536 x 256 KiB also run merkle_blocks + merkle_nodes beside merkle_uniform, "
                         "K alternating timed runs of each")
    ap.add_argument("--pieces-leg", type=int, default=0, metavar="K",
                    help="on 65,536 x 256 KiB and 1,024 x 4 MiB also run merkle_pieces (the fused kernel) beside "
                         "merkle_ragged (leaf + node), K alternating timed runs of each")
    ap.add_argument("--no-sha1", action="store_true", help="skip the SHA-1 kernel beside each shape (and the 2x condition)")
    args = ap.parse_args()

    isa = isa_valu_per_block(args.isa) if args.isa else None
    valu256 = isa["valu_per_block"] if isa else SHA256_VALU_PER_BLOCK

    import torch

    from vortex_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from vortex_amd import device as vdev

    if not torch.cuda.is_available():
        raise SystemExit("merkle_bench needs a GPU: a rate is a measurement on the device")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    simds = props.multi_processor_count * 4
    result = {"tool": "tools/merkle_bench.py", "label": args.label, "device": props.name,
              "compute_units": props.multi_processor_count, "hbm_peak_Bps": HBM_PEAK,
              "isa": isa or {"valu_per_block": SHA256_VALU_PER_BLOCK, "source": "DESIGN.md §3.7"},
              "sha1_valu_per_block": SHA1_VALU_PER_BLOCK, "shapes": []}
    ok = True
    for idx in (int(x) for x in args.shapes.split(",")):
        n, plen, sha1_kind = SHAPES[idx]
        log2_width = (plen // BLOCK).bit_length() - 1
        nbytes = n * plen
        data = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        vdev.synth_fill(data, n, plen, seed=0x5EED0256 + idx)
        leaves = torch.empty((n << log2_width, 32), dtype=torch.uint8, device=dev)
        roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)

        def merkle():
            vdev.merkle_uniform(data, n, plen, log2_width, leaves=leaves, roots=roots)

        merkle()
        torch.cuda.synchronize(dev)
        for i in (0, n - 1):  # what is timed computes the right thing
            piece = data[i * plen:(i + 1) * plen].cpu().numpy().tobytes()
            if roots[i].cpu().numpy().tobytes() != tree_root(piece, log2_width):
                raise SystemExit(f"{n} x {plen}: root of piece {i} differs from hashlib")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        merkle()
        e1.record()
        torch.cuda.synchronize(dev)
        steps = max(5, min(200, int(args.target_ms / max(e0.elapsed_time(e1), 1e-3))))
        t, clock = timed(merkle, args.warmup, steps, dev)
        shape = {"pieces": n, "piece_len": plen, "bytes": nbytes, "log2_width": log2_width,
                 "merkle": record(t, clock, nbytes, n << log2_width, BLOCK // 64, valu256, simds)}

        if idx == 0 and args.blocks_leg:
            # The block-stream kernel + the node entry over the same buffer,
            # rows piece-major so both write the same leaves: merkle_uniform
            # (unchanged code) and the pair alternate, --blocks-leg times each;
            # the spread between merkle_uniform's own runs is the margin.
            nb = n << log2_width
            b_rows = torch.arange(nb, dtype=torch.int32, device=dev)
            b_lens = torch.full((nb,), BLOCK, dtype=torch.int32, device=dev)
            b_leaves = torch.full((nb, 32), 0xFF, dtype=torch.uint8, device=dev)
            b_roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            vdev.merkle_blocks(data, b_rows, b_lens, b_leaves)  # validates the tables once

            def blocks():
                vdev.merkle_blocks(data, b_rows, b_lens, b_leaves, validate=False)
                vdev.merkle_nodes(b_leaves, n, log2_width, roots=b_roots)

            blocks()
            torch.cuda.synchronize(dev)
            if not (torch.equal(b_leaves, leaves) and torch.equal(b_roots, roots)):
                raise SystemExit(f"{n} x {plen}: blocks + nodes differ from merkle_uniform")
            runs = {"merkle_uniform": [], "blocks_nodes": []}
            for _ in range(args.blocks_leg):
                for name, fn in (("merkle_uniform", merkle), ("blocks_nodes", blocks)):
                    t, clock = timed(fn, args.warmup, steps, dev)
                    runs[name].append(record(t, clock, nbytes, nb, BLOCK // 64, valu256, simds))
            rates = {k: [r["GiB_per_s"] for r in v] for k, v in runs.items()}
            shape["blocks_leg"] = {
                "runs": runs, "GiB_per_s": rates,
                "merkle_uniform_spread": round(max(rates["merkle_uniform"]) - min(rates["merkle_uniform"]), 1),
                "blocks_minus_uniform_median": round(
                    sorted(rates["blocks_nodes"])[len(rates["blocks_nodes"]) // 2] -
                    sorted(rates["merkle_uniform"])[len(rates["merkle_uniform"]) // 2], 1)}
            del b_rows, b_lens, b_leaves, b_roots

        if idx in (0, 1) and args.pieces_leg:
            # The fused piece kernel (merkle_pieces: leaves reduced in LDS, no
            # leaf array) against the leaf + node pair (merkle_ragged) on the
            # same buffer, alternating; the spread between the pair's own runs
            # is the margin.
            p_offs = torch.arange(n, dtype=torch.int64, device=dev) * plen
            p_lens = torch.full((n,), plen, dtype=torch.int32, device=dev)
            r_roots = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            p_roots = torch.full((n, 32), 0xFF, dtype=torch.uint8, device=dev)
            vdev.merkle_ragged(data, p_offs, p_lens, log2_width, leaves=leaves, roots=r_roots)  # validates once

            def pair():
                vdev.merkle_ragged(data, p_offs, p_lens, log2_width, leaves=leaves, roots=r_roots, validate=False)

            def fused():
                vdev.merkle_pieces(data, p_offs, p_lens, log2_width, roots=p_roots, validate=False)

            fused()
            torch.cuda.synchronize(dev)
            if not (torch.equal(p_roots, roots) and torch.equal(r_roots, roots)):
                raise SystemExit(f"{n} x {plen}: merkle_pieces differs from the leaf + node pair")
            runs = {"merkle_ragged": [], "merkle_pieces": []}
            for _ in range(args.pieces_leg):
                for name, fn in (("merkle_ragged", pair), ("merkle_pieces", fused)):
                    t, clock = timed(fn, args.warmup, steps, dev)
                    runs[name].append(record(t, clock, nbytes, n << log2_width, BLOCK // 64, valu256, simds))
            rates = {k: [r["GiB_per_s"] for r in v] for k, v in runs.items()}
            med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
            shape["pieces_leg"] = {
                "runs": runs, "GiB_per_s": rates, "GiB_per_s_median": med,
                "merkle_ragged_spread": round(max(rates["merkle_ragged"]) - min(rates["merkle_ragged"]), 1),
                "pieces_minus_ragged_median": round(med["merkle_pieces"] - med["merkle_ragged"], 1)}
            del p_offs, p_lens, r_roots, p_roots

        if sha1_kind and not args.no_sha1:
            digests = torch.empty((n, 20), dtype=torch.uint8, device=dev)
            if sha1_kind == "sha1_uniform":
                def sha1():
                    vdev.sha1_uniform(data, n, plen, digests=digests)
            else:
                offsets = torch.arange(n, dtype=torch.int64, device=dev) * plen
                lens = torch.full((n,), plen, dtype=torch.int32, device=dev)
                vdev.sha1_ragged(data, offsets, lens, digests=digests, plan=(plen, nbytes))  # validates the layout once

                def sha1():
                    vdev.sha1_ragged(data, offsets, lens, digests=digests, plan=(plen, nbytes), validate=False)
            sha1()
            torch.cuda.synchronize(dev)
            piece = data[:plen].cpu().numpy().tobytes()
            if digests[0].cpu().numpy().tobytes() != hashlib.sha1(piece).digest():
                raise SystemExit(f"{n} x {plen}: SHA-1 of piece 0 differs from hashlib")
            e0.record()
            sha1()
            e1.record()
            torch.cuda.synchronize(dev)
            steps = max(5, min(200, int(args.target_ms / max(e0.elapsed_time(e1), 1e-3))))
            t, clock = timed(sha1, args.warmup, steps, dev)
            shape[sha1_kind] = record(t, clock, nbytes, n, plen // 64, SHA1_VALU_PER_BLOCK, simds)
            shape["merkle_over_sha1"] = round(shape["merkle"]["GiB_per_s"] / shape[sha1_kind]["GiB_per_s"], 3)
            if sha1_kind == "sha1_ragged":
                shape["condition"] = {"merkle_over_sha1_ragged_min": 2.0,
                                      "met": shape["merkle_over_sha1"] >= 2.0}
                ok = ok and shape["condition"]["met"]
        result["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
        del data, leaves, roots
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        print("merkle path is under 2x the SHA-1 ragged rate on 1,024 x 4 MiB", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
