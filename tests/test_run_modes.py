"""The run's mode resolver (csrc/hip/gss_run_modes.h) alone, on the CPU.

tests/helpers/run_modes_check.cpp includes only that header: a table of named cases (defaults at
small and large slots, every switch that changes a mode, the carrier hand-off with and without a
prediction callback, the integer carrier) against the modes the documentation gives for them,
and the invariants gss_run.hip relies on over the whole product of switch values.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_modes(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "run_modes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "gps-sdr-sim_amd", "csrc", "hip"),
                    os.path.join(ROOT, "tests", "helpers", "run_modes_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all cases ok" in r.stdout
    assert "FAIL" not in r.stdout
