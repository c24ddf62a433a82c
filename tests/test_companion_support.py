"""The host support the eight companion libraries share
(hadoofus_amd/csrc/companion_support.h; grid_segments and timed_frame_run of
wire_layout.h; the fused libraries' device state of wire_fused_host.h; the
batch front end of wire_batch_layout.h), on the CPU:
tests/consumer/companion_selftest.cpp defines a fake HIP runtime and a fake
engine that count and log every call and can be told to fail, and is built
with ASan/UBSan against the ROCm headers alone (it is not linked to the
runtime).  It covers the error and lifetime paths the GPU tests cannot reach
-- failed allocations, streams and events, a failing kernel preparation, a
change of the engine's device -- and pins the runtime calls of a warm call:
none from the buffers, the table pair, the events, the fused state and the
scratch, one attributes and one range query per allocation, and the exact
sequence of the frame run.  The overlap sweep of a batch's buffers is checked
against a scan of every pair, over every small batch and a few thousand random
ones."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(d, "include")
    return None


@pytest.mark.skipif(_rocm_include() is None, reason="the ROCm headers are not installed")
def test_companion_support_selftest(tmp_path):
    exe = tmp_path / "companion_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "companion_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout
