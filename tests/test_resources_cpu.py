"""CPU: the handles that own the engine's device and pinned blocks, streams,
events and stages (vortex_amd/csrc/vx_resources.hpp), run as a stand-alone
program under ASan + UBSan over a fake runtime: tests/native/resources_check.cpp
defines the handles' backend over malloc and a log of calls.  The header takes
HIP's types from hip_runtime_api.h and nothing else, so plain g++ builds the
program and no HIP library is linked.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_handles_over_a_fake_runtime(tmp_path):
    """Per handle type: move construction, move assignment onto an empty and a
    non-empty target (the target's old resource is released exactly once),
    self-move, reset twice, a failed creation.  reserve: equal or smaller does
    nothing, larger frees and then allocates, a failing allocation leaves the
    handle empty with size 0 and a later reserve works.  A vector of structs of
    the four handles through a reallocation, resize down, assignment of an
    empty element and clear: every resource is released once.  A struct
    {block, event, stream} goes as: synchronize stream, destroy stream, destroy
    event, free block.  The stage: the 2 MiB-aligned registered mapping, the
    fallback to pinned memory when registration is refused, and its moves.
    Nothing is alive at exit (the fake runtime's own count, and ASan's leak
    check)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "resources_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "vortex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "resources_check.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["failures"] == 0 and got["checks"] >= 100, got
