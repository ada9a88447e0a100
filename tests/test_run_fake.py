"""gss_run (csrc/hip/gss_run.hip, gss_run_plan.hip and gss_run_pool.hip with their headers, as
shipped) on the CPU fake of the HIP runtime.

tests/helpers/fake_hip stands in for the HIP calls gss_run makes (streams drained by worker
threads, events as generation counters), tests/helpers/fake_dev.cpp for its device functions
(renders write a fingerprint of each block's rows and nav words), and run_fake.cpp drives
every mode of the run (host / gpu / split proofs, GSS_PATH=walk, two runs on one handle, the two-rank
baton hand-off, a sink that stops) checking every byte the sink receives.  tools/sanitize.sh
runs the same program under TSan and ASan+UBSan; this is the plain build, so the CPU suite
catches an orchestration regression without a GPU.
"""
import os
import subprocess

import pytest

from fake_build import programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAV = os.path.join(ROOT, "tests", "golden", "data", "brdc3540.14n")


@pytest.fixture(scope="module")
def run_fake(tmp_path_factory):
    return programs(tmp_path_factory, "run_fake", nolaunch=False)["run_fake"]


@pytest.mark.parametrize("args", [("35", "64", "1"), ("25", "16", "8")])
def test_gss_run_on_fake_device(run_fake, args):
    r = subprocess.run([run_fake, NAV, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all modes ok" in r.stdout
