"""bench.py's multi-GPU contract (VERDICT r2 "Next round" 1).

* CPU: `bench.py --gpus N` under a launcher must have WORLD_SIZE == N, and a
  plain `bench.py --gpus N` that cannot start N ranks fails non-zero without
  printing a result line — it never reports a one-GPU run for --gpus N.
* GPU: a plain `bench.py --gpus 2` (gloo, both ranks on the box's one GPU)
  launches its own two ranks and prints one line with n_gpus = world_size = 2;
  under torch.distributed.run with one rank the process group is RCCL
  ("nccl") at world size 1, so RCCL init and the device-tensor all-gather of
  the verdicts run on hardware.
* A plain run measures the headline only (extra legs need --full), and
  --dump-outputs writes the last timed step's verdicts as float32 .npy files.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--pieces", "1024", "--steps", "3", "--warmup", "1", "--no-e2e", "--no-ragged", "--no-reverify",
         "--no-cpu-baseline"]


def _run(args, env_extra=None, timeout=300):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env)


def _lines(out: str):
    return [json.loads(x) for x in out.splitlines() if x.startswith("{")]


def _check_line_size(out: str):
    """The result line the driver parses stays within bench.LINE_LIMIT (8 KB)."""
    (line,) = [x for x in out.splitlines() if x.startswith("{")]
    assert len(line.encode()) <= 8192, len(line)


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "2"] + SMALL, {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"}, timeout=120)
    assert r.returncode != 0 and not _lines(r.stdout)
    assert "WORLD_SIZE 3" in r.stderr


def test_launch_command_shape():
    sys.path.insert(0, ROOT)
    import argparse

    import bench

    args = argparse.Namespace(gpus=8, same_device=False)
    cmd = bench.launch_cmd(args, ["--gpus", "8", "--steps", "5"], 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--master-addr=127.0.0.1" in cmd and "--master-port=29555" in cmd
    assert cmd[-3:] == ["--gpus", "8", "--steps", "5"][-3:] and os.path.abspath(BENCH) in cmd


def test_plain_multi_gpu_run_without_gpus_fails_loudly():
    """No KFD topology here (or fewer GPUs than asked): refuse before launching."""
    from vortex_amd import topology

    n = topology.visible_gpus()
    if n is not None and n >= 2:
        pytest.skip("GPUs visible")
    r = _run(["--gpus", "2"] + SMALL, timeout=120)  # counts devices from sysfs, refuses before launching
    assert r.returncode == 2 and not _lines(r.stdout)
    assert "refusing" in r.stderr
    if not n:
        # rehearsal form: both ranks would share cuda:0; with no GPU the ranks die and so does the run
        r = _run(["--gpus", "2", "--same-device", "--dist-backend", "gloo"] + SMALL, timeout=240)
        assert r.returncode != 0 and not _lines(r.stdout)


def _fake_kfd(tmp_path, nodes, renders):
    """A KFD topology tree: nodes = [(gfx_target_version, drm_render_minor) or None (no properties)]."""
    kfd = tmp_path / "nodes"
    dri = tmp_path / "dri"
    dri.mkdir()
    for k, nd in enumerate(nodes):
        d = kfd / str(k)
        d.mkdir(parents=True)
        if nd is not None:
            gfx, minor = nd
            (d / "properties").write_text(f"cpu_cores_count 0\nsimd_count 1024\ngfx_target_version {gfx}\n"
                                          f"drm_render_minor {minor}\nlocation_id {4096 * k}\n")
    for m in renders:
        (dri / f"renderD{m}").write_text("")
    return str(kfd), str(dri)


def test_topology_count_from_sysfs(tmp_path):
    """vortex_amd.topology counts GPU nodes (gfx_target_version != 0) whose
    render node exists here and whose properties are readable, capped by every
    *_VISIBLE_DEVICES variable that is set; CPU nodes never count."""
    from vortex_amd import topology

    # node 0: CPU; 1-4: GPUs, of which render 131 is not in this container; 5: properties hidden (cgroup)
    kfd, dri = _fake_kfd(tmp_path, [(0, 0), (90500, 128), (90500, 129), (90500, 130), (90500, 131), None],
                         [128, 129, 130])
    assert topology.visible_gpus(kfd, dri, environ={}) == 3
    assert [g["drm_render_minor"] for g in topology.kfd_gpus(kfd, dri)] == [128, 129, 130]
    assert topology.visible_gpus(kfd, dri, environ={"HIP_VISIBLE_DEVICES": "0,1"}) == 2
    assert topology.visible_gpus(kfd, dri, environ={"ROCR_VISIBLE_DEVICES": "1", "HIP_VISIBLE_DEVICES": "0,1"}) == 1
    assert topology.visible_gpus(kfd, dri, environ={"CUDA_VISIBLE_DEVICES": ""}) == 0
    assert topology.visible_gpus(str(tmp_path / "absent"), dri, environ={}) is None


def test_launcher_parent_never_maps_hip():
    """The parent's whole pre-launch path (sysfs count, refusal) runs without
    the HIP runtime in the process (the same check launch_ranks makes before
    it starts the launcher)."""
    code = ("import sys; sys.argv = ['bench.py', '--gpus', '64'] + %r; import bench; rc = bench.main(); "
            "from vortex_amd import topology; print('MAPPED' if topology.hip_runtime_mapped() else 'CLEAN', rc)"
            % SMALL)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert r.stdout.split() == ["CLEAN", "2"], (r.stdout, r.stderr[-2000:])


@pytest.mark.gpu
def test_plain_multi_gpu_refused_on_one_gpu_box(built, gpu):
    """On the 1-GPU box a plain `bench.py --gpus 2` (no --same-device) must be
    refused from the sysfs count — rc 2, no result line — by a parent that
    never mapped the HIP runtime, and the sysfs count must equal what HIP sees
    (torch, in this test process)."""
    import torch

    from vortex_amd import topology

    assert topology.visible_gpus() == torch.cuda.device_count() == 1
    r = _run(["--gpus", "2"] + SMALL, timeout=120)
    assert r.returncode == 2 and not _lines(r.stdout), r.stderr[-2000:]
    assert "only 1 GPU(s) visible" in r.stderr
    test_launcher_parent_never_maps_hip()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 8])
def test_plain_bench_launches_its_ranks(built, gpu, n, tmp_path):
    """n = 8 rehearses config 4's shape on the one-GPU box: 8 ranks, global
    piece indices r*1024 + i, the verdicts of all 8 shards gathered and the
    exact 1 % mismatch set checked on the gathered table."""
    side = tmp_path / "detail.json"
    r = _run(["--gpus", str(n), "--same-device", "--dist-backend", "gloo", "--detail", str(side), "--full",
              "--dump-outputs", str(tmp_path / "out")] + SMALL,
             timeout=300)  # --full: the verdict gather alone is timed too (verdict_gather_ms)
    assert r.returncode == 0, r.stderr[-3000:]
    import numpy as np

    # rank 0's own verdicts and the gathered table of the last timed step: every 100th global piece is corrupt
    want = np.array([0.0 if i % 100 == 99 else 1.0 for i in range(n * 1024)], dtype=np.float32)
    assert np.array_equal(np.load(tmp_path / "out" / "matched.npy"), want[:1024])
    assert np.array_equal(np.load(tmp_path / "out" / "verdicts.npy"), want)
    (res,) = _lines(r.stdout)
    _check_line_size(r.stdout)
    assert res["detail"] == str(side)
    assert res["n_gpus"] == n and res["world_size"] == n and res["backend"] == "gloo"
    assert res["value"] > 0 and res["config"]["pieces_per_gpu"] == 1024
    assert res["config"]["total_GiB"] == n * 1024 * 256 / (1 << 20)
    rk = res["ranks"]  # every rank's step, kernel and verdict-gather times
    assert all(len(rk[k]) == n for k in ("step_ms", "kernel_ms", "verdict_gather_ms"))
    assert max(rk["step_ms"]) == pytest.approx(res["ms_per_step"], rel=1e-3)
    # identity: every rank names its device (in full in the side file); all share the one GPU here,
    # and the line says so
    full = json.loads(side.read_text())
    devs = full["ranks"]["devices"]
    assert [d["rank"] for d in devs] == list(range(n)) and rk["pci_bus_ids"] == [d["pci_bus_id"] for d in devs]
    assert all(d["world_size"] == n and d["pci_bus_id"] == devs[0]["pci_bus_id"] for d in devs)
    assert rk["distinct_devices"] is False and full["value"] == res["value"]
    assert all(1.0 < g < 3.0 for g in rk["clock_GHz"])
    # every gathered verdict checked, clean pieces against the CPU pool's digests
    assert res["parity"]["checked"] == n * 1024 and res["config"]["parity_checked"] == n * 1024
    corrupt = sum(1 for i in range(n * 1024) if i % 100 == 99)
    assert res["parity"]["corrupt_mismatched"] == corrupt and res["parity"]["bit_exact"] == n * 1024 - corrupt


def test_steps_must_be_positive():
    """--steps sets the number of timed steps; none is refused before anything runs."""
    r = _run(["--gpus", "1", "--steps", "0"], timeout=60)
    assert r.returncode == 2 and not _lines(r.stdout) and "--steps" in r.stderr


def test_dump_outputs_writes_float32_within_the_limit(tmp_path):
    """bench.dump_outputs: every array as float32 <name>.npy; arrays over their
    share of the byte limit are cut to the same seeded sample on every call."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    small = np.arange(1000, dtype=np.uint8) % 2
    big = np.arange(5000, dtype=np.int64)
    for d in ("a", "b"):
        wrote = bench.dump_outputs(str(tmp_path / d), {"matched": small, "verdicts": big}, limit=16000)
        assert wrote == {"matched": 1000, "verdicts": 2000}  # 16,000 B = 2 x 2,000 float32
    a, b = (np.load(tmp_path / d / "verdicts.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (2000,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a.tolist()) <= set(range(5000))  # a sorted subset, no repeats
    m = np.load(tmp_path / "a" / "matched.npy")
    assert m.dtype == np.float32 and np.array_equal(m, small.astype(np.float32))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 16000 + 2 * 128


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_verdicts(built, gpu, tmp_path):
    """A plain run (no --full, no --no-* option) times exactly --steps steps and
    measures no extra leg; --dump-outputs holds the last timed step's verdicts
    as float32: 0.0 for exactly the corrupted pieces (every 100th), else 1.0."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    side, out = tmp_path / "detail.json", tmp_path / "out"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--pieces", "1024", "--detail", str(side),
              "--dump-outputs", str(out)], timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    (res,) = _lines(r.stdout)
    _check_line_size(r.stdout)
    full = json.loads(side.read_text())
    for rec in (res, full):
        assert not [k for k in bench.LEGS + ("cpu_baseline",) if k in rec], sorted(rec)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["dtype"] == "u32"
    assert res["ms_per_step"] > 0 and res["higher_is_better"] is True and res["unit"] == "GiB/s"
    assert res["value"] == pytest.approx(1024 * 262144 / (res["ms_per_step"] * 1e-3) / (1 << 30), rel=1e-2)
    assert res["roofline"]["kernel_ms"] > 0 and res["parity"]["checked"] == 1024
    assert os.listdir(out) == ["matched.npy"]
    m = np.load(out / "matched.npy")
    assert m.dtype == np.float32 and m.shape == (1024,)
    assert np.array_equal(m, np.array([0.0 if i % 100 == 99 else 1.0 for i in range(1024)], dtype=np.float32))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_config4_full_size_8_ranks(built, gpu, tmp_path):
    """BASELINE config 4 at full size on the box's one GPU: 8 gloo ranks x
    65,536 x 256 KiB = 524,288 pieces (128 GiB in one GPU's HBM), global piece
    indices r*65536 + i.  Each rank's expected table is the CPU pool
    restatement's digests of its clean pieces (oracle/pool_oracle.cpp, the
    par_iter of torrent.rs:724-740 split by index), so the check on the
    gathered table — exactly the 1 % corrupted pieces mismatch — proves all
    519,046 clean digests bit-exact against vortex's pool."""
    args = ["--gpus", "8", "--same-device", "--dist-backend", "gloo", "--pieces", "65536", "--steps", "2",
            "--warmup", "1", "--no-e2e", "--no-ragged", "--no-reverify", "--no-cpu-baseline",
            "--detail", str(tmp_path / "detail.json")]
    r = _run(args, timeout=840)
    assert r.returncode == 0, r.stderr[-3000:]
    (res,) = _lines(r.stdout)
    _check_line_size(r.stdout)  # the N=8 shape the driver's 8-GPU node prints
    assert len(res["ranks"]["pci_bus_ids"]) == 8 and res["roofline"]["frac"] > 0
    assert res["n_gpus"] == 8 and res["world_size"] == 8 and res["config"]["pieces_per_gpu"] == 65536
    assert res["config"]["total_GiB"] == 128.0
    p = res["parity"]
    corrupt = sum(1 for i in range(8 * 65536) if i % 100 == 99)
    assert p["checked"] == 524288 and p["corrupt_mismatched"] == corrupt and p["bit_exact"] == 524288 - corrupt
    assert res["config"]["parity_checked"] == 524288


@pytest.mark.gpu
def test_bench_rccl_world_size_1(built, gpu, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr=127.0.0.1", f"--master-port={port}", BENCH, "--gpus", "1"] + SMALL \
        + ["--full", "--detail", str(tmp_path / "detail.json")]  # --full: verdict_gather_ms
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    (res,) = _lines(r.stdout)
    _check_line_size(r.stdout)  # the RCCL line prints the compact form too
    full = json.loads((tmp_path / "detail.json").read_text())
    assert res["n_gpus"] == 1 and res["world_size"] == 1 and res["backend"] == "nccl"
    assert "nccl all-gather of verdicts" in res["config"]["workload"]
    assert len(res["ranks"]["verdict_gather_ms"]) == 1 and res["ranks"]["verdict_gather_ms"][0] > 0
    assert res["ranks"]["distinct_devices"] is True and full["ranks"]["devices"][0]["world_size"] == 1
    assert "valu" not in res["roofline"]
    clk = full["roofline"]["valu"]["clock_run"]
    assert 1.0 < clk["GHz_mean"] < 3.0 and 0 < clk["kernel_busy_frac"] <= 1.0
    frac = clk["one_wave_issue_at_run_clock"]["frac"]  # null when gathers fill > 0.1 of the stamped span
    assert (frac is None) == (clk["kernel_busy_frac"] < 0.9) and (frac is None or frac > 0)
    assert res["roofline"]["clock_GHz_run"] == clk["GHz_mean"]


@pytest.mark.gpu
def test_reverify_multi_leg_rccl_world_size_1(built, gpu, tmp_path):
    """The N>1 config-5 leg on RCCL (verdicts gathered on the device, identity
    and times through nccl's all_gather_object), at the one world size the box
    allows for RCCL: what the driver's 8-GPU run takes, minus the other ranks."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    args = ["--pieces", "1024", "--steps", "2", "--warmup", "1", "--no-e2e", "--no-ragged", "--no-cpu-baseline",
            "--reverify-multi", "--reverify-multi-scale", "0.05", "--detail", str(tmp_path / "detail.json")]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr=127.0.0.1", f"--master-port={port}", BENCH, "--gpus", "1"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    (line,) = _lines(r.stdout)
    _check_line_size(r.stdout)
    res = json.loads((tmp_path / "detail.json").read_text())
    assert line["reverify_multi"]["warm.value"] == res["reverify_multi"]["warm"]["value"]
    assert res["backend"] == "nccl" and "reverify" not in res
    rm = res["reverify_multi"]
    assert "error" not in rm, rm
    assert rm["ranks"] == 1 and rm["same_device"] is False and rm["cpu_pool_verdicts_ok"] is True
    assert rm["pieces"] == 70
    for leg in ("warm", "cold"):
        assert rm[leg]["value"] > 0 and all(len(t) == 1 for t in rm[leg]["rank_traces"])
    _check_plan(rm)


def test_clock_from_stamps():
    """Per-XCC clock = shader cycles / real-time ticks x the tick rate, each XCC
    against its own counters (their offsets differ)."""
    sys.path.insert(0, ROOT)
    import bench

    before, after = [], []
    for b in range(16):
        x = b % 8
        off = 10 ** 12 * x  # XCCs' cycle counters disagree by a constant
        ghz = 2.0 + 0.05 * x
        before.append((off + 1000, 5_000, x))
        after.append((off + 1000 + int(ghz * 1e9 * 0.1), 5_000 + 10_000_000, x))  # 0.1 s at 100 MHz
    r = bench.clock_from_stamps(before, after, 100_000)
    assert r["GHz_per_xcc"]["0"] == pytest.approx(2.0, rel=1e-6)
    assert r["GHz_per_xcc"]["7"] == pytest.approx(2.35, rel=1e-6)
    assert r["GHz_mean"] == pytest.approx(2.175, rel=1e-4) and r["span_ms"] == pytest.approx(100.0)


@pytest.mark.gpu
def test_reverify_multi_leg_rehearsal(built, gpu, tmp_path):
    """The N>1 line's config-5 leg (bench.reverify_multi_leg), rehearsed with 2
    gloo ranks on the box's one GPU and 5 % of linux-mint's pieces: every rank
    verifies its piece range on its GPU, the slowest rank's time is the call's,
    every verdict is gathered and checked (a wrong one raises on every rank),
    and the CPU pool restatement runs beside it with every host CPU."""
    args = ["--pieces", "1024", "--steps", "2", "--warmup", "1", "--no-e2e", "--no-ragged", "--no-cpu-baseline",
            "--gpus", "2", "--same-device", "--dist-backend", "gloo", "--reverify-multi",
            "--reverify-multi-scale", "0.05", "--detail", str(tmp_path / "detail.json")]
    r = _run(args, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_line_size(r.stdout)
    res = json.loads((tmp_path / "detail.json").read_text())
    rm = res["reverify_multi"]
    assert "error" not in rm, rm
    assert rm["ranks"] == 2 and rm["same_device"] is True and rm["cpu_pool_verdicts_ok"] is True
    assert rm["pieces"] == 70 and rm["bytes"] == 69 * 2097152 + 1179648
    for leg in ("warm", "cold"):
        assert rm[leg]["value"] > 0 and rm[leg]["cpu_pool"]["value"] > 0
        assert all(len(t) == 2 for t in rm[leg]["rank_traces"])
    _check_plan(rm)
    _check_split(rm)
    _check_balanced(rm)


def _check_split(rm):
    """The node-level split (bench.multi_split): the planner's GPU tail over the
    ranks, rank 0's pool on the head, one time per call, every verdict checked."""
    sp = rm["split"]
    assert sp["gpu_first"] + sp["gpu_count"] == rm["pieces"] and sp["value"] > 0 and len(sp["s_runs"]) >= 1
    assert sp["gpu_first"] == sp["plan"]["gpu_first"] and isinstance(sp["beats_both"], bool)


def _check_balanced(rm):
    """The node-level balanced split (bench.multi_balanced): one claim word in
    /dev/shm for every rank's engine and rank 0's pool, every verdict checked."""
    b = rm["split_balanced"]
    assert b["value"] > 0 and len(b["s_runs"]) >= 1 and all(0 <= g <= rm["pieces"] for g in b["gpu_first_runs"])


def _check_plan(rm):
    """The record's model prediction: one 2 MiB piece's chain floors the call."""
    p = rm["plan"]
    assert 0.02 < p["gpu_chain_s"] < 0.03 and p["gpu_s"] >= p["gpu_chain_s"]
    assert p["cpu_s"] > 0 and isinstance(p["use_gpu"], bool) and p["predicted_GiBps"] > 0


@pytest.mark.parametrize("mode", ["ok", "fail"])
def test_reverify_multi_leg_collective_logic_cpu(tmp_path, mode):
    """bench.reverify_multi_leg at world size 2 on gloo, no GPU: the engine is
    replaced by a CPU stand-in that verifies each rank's piece range with the
    oracle (tests/_multi_leg_rank.py).  "ok": rank 0 reports warm and cold
    rates from the slowest rank, every verdict gathered.  "fail": rank 1's
    second timed call raises; both ranks must raise together (no rank left
    waiting in a collective) and the file must be gone."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = tmp_path / "out.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", TMPDIR=str(tmp_path))
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "tests", "_multi_leg_rank.py"),
           str(out), mode]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(out.read_text())
    if mode == "ok":
        rm = d["result"]
        assert rm["ranks"] == 2 and rm["pieces"] == 28 and rm["cpu_pool_verdicts_ok"] is True
        for leg in ("warm", "cold"):
            assert rm[leg]["value"] > 0 and all(len(t) == 2 for t in rm[leg]["rank_traces"])
        _check_plan(rm)
        _check_split(rm)
        _check_balanced(rm)
    else:
        assert "vx_verify_files_range call failed" in d["error"]
    assert not [p for p in os.listdir(tmp_path) if p.startswith("vx_bench_multi_linuxmint")]


def test_node_cpus_honours_cgroup_quota(tmp_path):
    """The multi-GPU leg sizes its readers and CPU pool from the affinity set
    capped by a cgroup v2 quota, not from OMP_NUM_THREADS (torchrun sets it
    to 1 per rank)."""
    sys.path.insert(0, ROOT)
    import bench

    aff = len(os.sched_getaffinity(0))
    q = tmp_path / "cpu.max"
    q.write_text("max 100000\n")
    assert bench.node_cpus(str(q)) == aff
    q.write_text("200000 100000\n")
    assert bench.node_cpus(str(q)) == min(aff, 2)
    q.write_text("50000 100000\n")
    assert bench.node_cpus(str(q)) == 1
    assert bench.node_cpus(str(tmp_path / "absent")) == aff


def test_disk_direct_rate_reads_the_whole_file(tmp_path):
    """The cold leg's disk reference (bench.disk_direct_rate): O_DIRECT reads
    of the evicted file in 1 MiB blocks, a ragged tail included, counted only
    when every byte came back; None where the filesystem refuses O_DIRECT."""
    sys.path.insert(0, ROOT)
    import bench

    size = (3 << 20) + 4097
    p = tmp_path / "f.bin"
    p.write_bytes(os.urandom(size))
    bench.drop_cache(str(p))
    r = bench.disk_direct_rate(str(p), size, 3)
    assert r is None or r > 0
    if r is not None:  # a wrong total is never reported as a rate
        assert bench.disk_direct_rate(str(p), size + 1, 3) is None


def test_roofline_scalars_for_the_record():
    """The driver keeps only the scalar fields of `roofline`: the clock the
    run held and the kernel's fraction of its binding (VALU-issue) roof must
    be top-level scalars there, not only inside the nested `valu` dict."""
    sys.path.insert(0, ROOT)
    import bench

    clock = {"GHz_mean": 2.2, "GHz_min": 2.1, "GHz_max": 2.3, "span_ms": 100.0, "GHz_per_xcc": {}}
    r = bench.roofline(65536, 262144, 4.9, 65536 * 262144 / 4.9e-3, "w", clock, steps=20)
    for k in ("bound", "achieved", "peak", "unit", "frac", "kernel_ms", "algorithmic_bytes_per_launch",
              "clock_GHz_run", "clock_GHz_run_min", "clock_kernel_busy_frac", "valu_Tops",
              "valu_issue_frac_run_clock", "valu_issue_frac_nominal"):
        assert isinstance(r[k], (int, float, str)) and not isinstance(r[k], bool), k
    assert r["clock_GHz_run"] == 2.2 and r["clock_GHz_run_min"] == 2.1
    assert r["clock_kernel_busy_frac"] == pytest.approx(0.98)
    ops = 65536 * 4097 * 613.5 / 4.9e-3
    assert r["valu_issue_frac_run_clock"] == pytest.approx(ops / (1024 * 16 * 2.2e9), abs=1e-4)
    assert r["valu_issue_frac_nominal"] == pytest.approx(ops / (1024 * 16 * 2.4e9), abs=1e-4)
    # a span the kernels fill only half of (gathers, N > 1): the mean clock is not theirs
    r2 = bench.roofline(65536, 262144, 4.9, 1.0, "w", dict(clock, span_ms=196.0), steps=20)
    assert r2["clock_kernel_busy_frac"] == pytest.approx(0.5) and r2["valu_issue_frac_run_clock"] is None


# The keys the record must carry in the parsed line (VERDICT r5 "Next round" 1).
ROOF_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_ratio", "kernel_ms",
             "algorithmic_bytes_per_launch", "clock_GHz_run", "clock_GHz_run_min", "clock_kernel_busy_frac",
             "valu_Tops", "valu_issue_frac_run_clock", "valu_issue_frac_nominal")
HEAD_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
             "vs_baseline", "dtype", "data", "config", "roofline", "parity", "cpu_baseline")


def _record_line(path):
    with open(os.path.join(ROOT, path)) as f:
        return json.loads([x for x in f if x.startswith("{")][-1])


def test_compact_line_of_round5_record():
    """Round 5's 23 KB line (profiles/r05/bench_head.json) through the same
    compaction bench.py now applies: ≤ 8 KB, every key the record is read
    for, roofline scalars only, each leg's value, the split's figures."""
    sys.path.insert(0, ROOT)
    import bench

    full = _record_line("profiles/r05/bench_head.json")
    assert len(json.dumps(full)) > 20000
    line = bench.compact_line(full, "bench_detail.json")
    text = json.dumps(line)
    assert len(text.encode()) <= 8192
    for k in HEAD_KEYS:
        assert k in line, k
    for k in ROOF_KEYS:
        assert line["roofline"][k] == full["roofline"][k], k
    assert not any(isinstance(v, (dict, list)) for v in line["roofline"].values())
    assert line["cpu_baseline"] == full["cpu_baseline"] and line["parity"] == full["parity"]
    assert line["value"] == full["value"] and line["config"] == full["config"]
    for leg in bench.LEGS:
        if leg in full:
            assert line[leg]["value"] == full[leg]["value"], leg
    assert line["reverify"]["split.value"] == full["reverify"]["split"]["value"]
    assert line["reverify"]["split.best_value"] == full["reverify"]["split"]["best_value"]
    assert line["reverify_cold"]["disk_direct.value"] == full["reverify_cold"]["disk_direct"]["value"]
    assert line["reverify"]["cpu_pool.value"] == full["reverify"]["cpu_pool"]["value"]
    assert "gpu_traces" not in text and "timeline" not in text and line["detail"] == "bench_detail.json"


def test_compact_line_of_8_rank_shape():
    """The N=8 shape (round 4's 8-rank line plus a reverify_multi leg): per-rank
    lists and bus ids stay, identities go to the side file, ≤ 8 KB."""
    sys.path.insert(0, ROOT)
    import bench

    full = _record_line("profiles/r04/round_end_head/bench_8rank.json")
    assert len(full["ranks"]["devices"]) == 8
    full["reverify_multi"] = {"warm": {"value": 150.0, "rank_traces": [[{"wall_ms": 1.0}] * 8] * 5,
                                       "cpu_pool": {"value": 30.0}},
                              "cold": {"value": 40.0}, "ranks": 8, "pieces": 1387,
                              "split": {"value": 160.0, "s_runs": [0.02] * 7, "sample": "x" * 400}}
    line = bench.compact_line(full, "bench_detail.json")
    assert len(json.dumps(line).encode()) <= 8192
    rk = line["ranks"]
    assert len(rk["step_ms"]) == 8 and len(rk["pci_bus_ids"]) == 8 and "devices" not in rk
    assert line["reverify_multi"]["warm.value"] == 150.0 and line["reverify_multi"]["split.value"] == 160.0
    for k in ("metric", "value", "n_gpus", "roofline", "config"):  # (round 4's line had no `parity` yet)
        assert k in line


def test_compact_line_never_drops_the_headline():
    """Legs that stay too large even as scalars are cut down, in steps, to
    value/error and then away; the headline, roofline, cpu_baseline and
    parity always print."""
    sys.path.insert(0, ROOT)
    import bench

    full = _record_line("profiles/r05/bench_head.json")
    big = {f"k{i}": float(i) for i in range(400)}
    for leg in ("ragged", "e2e", "reverify"):
        full[leg] = dict(big, value=1.5, error=None)
    line = bench.compact_line(full, None)
    assert len(json.dumps(line).encode()) <= 8192
    assert line["ragged"] == {"value": 1.5} and "detail" not in line
    full["e2e_async"] = {"error": "E" * 5000}
    line = bench.compact_line(full, None)
    assert len(line["e2e_async"]["error"]) == 240
    full["ragged"] = {"value": 1.0, "unit": "u" * 9000}
    line = bench.compact_line(full, None)
    assert "ragged" not in line and all(k in line for k in HEAD_KEYS)
