"""The run's stage resolver (csrc/hip/gss_run_stages.h) with the host plane alone, on the CPU.

tests/helpers/run_stages_check.cpp includes only that header: named cases for every refusal of
run_stages_resolve (code, text, and which refusal comes first) and for the formats, block sizes,
second slot buffer and lead blocks it resolves: noise at SC16, SC08 and SC01, with and without a
filter, ranges from block 0, block 1 and past the filter's memory, blocks shorter than that
memory, an empty range.  It links the host objects of the session's fake build (fake_build.py).
"""
import os
import shutil
import subprocess

import pytest

from fake_build import CF, common_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_stages(tmp_path, tmp_path_factory):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("gcc/g++ not available")
    _, objs = common_objects(tmp_path_factory)
    host = [o for o in objs
            if not os.path.basename(o).startswith(("gss_run", "fake_hip", "fake_dev"))]
    exe = str(tmp_path / "run_stages_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + CF +
                   ["-I" + os.path.join(ROOT, "gps-sdr-sim_amd", "csrc", "hip"),
                    os.path.join(ROOT, "tests", "helpers", "run_stages_check.cpp")] + host +
                   ["-o", exe, "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all cases ok" in r.stdout
    assert "FAIL" not in r.stdout
