"""CPU: the round driver of the v2 and hybrid files calls
(vortex_amd/csrc/vx_block_rounds.hpp), run as a stand-alone program under
ASan + UBSan with the real reader pool and the real round planners over a fake
device (tests/native/block_rounds_check.cpp).  The header has no HIP in it: the
program is built by plain g++ with no ROCm include path.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_slot_ring_over_a_fake_device(tmp_path):
    """nslots in {1, 2, 3, 5} x lag in {0, 1, 7, never} x both planners at rounds
    of 4 and 16 blocks, a v2 run over holes and a planner without a round: the
    rounds are enqueued in planner order, round k on slot k % nslots, the totals
    are the sums over the rounds, never more than nslots rounds lie between
    read-submitted and completed, every read is in its stage at enqueue and no
    read lands in a stage whose copy is in flight.  Then the stage request, the
    enqueue and the done-query each fail at the first, a middle and the last
    round: the driver returns that code with exactly the rounds before it
    enqueued, none after it and no read outstanding."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "block_rounds_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "block_rounds_check.cpp"), "-o", str(exe), "-lpthread"],
                   check=True)
    data = tmp_path / "data"
    data.mkdir()
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    # 2 planners x 2 round sizes x 4 slot counts x 4 lags, holes, the empty planner; 2 planners x 2 x 2 x 3 x 3 failures
    assert got == {"sweeps": 66, "failures": 72, "mismatches": 0, "errors": 0}, got
