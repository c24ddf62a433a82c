"""The tune word and the static tile dealing (hadoofus_amd/csrc/crc32c_deal.h).

tiles_run takes its static schedule, and the speculative batch kernel the
tiles of each run a workgroup owns (which decide when a run's verdict is
published), from one host-and-device function.  CPU: that function against a
brute-force walk of every workgroup's static tickets, over every dealing
(tests/consumer/deal_selftest.cpp, built with ASan/UBSan, nothing loaded
into Python).  GPU: tests/test_jobs_early.py runs the dealings through the
diagnostic build's device check."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deal_selftest(tmp_path):
    exe = tmp_path / "deal_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "deal_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout
    print(p.stdout)
