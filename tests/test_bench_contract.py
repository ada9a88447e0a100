"""bench.py pieces that need no GPU: the metric is BASELINE.json's, the committed PMC traffic
record (profiles/pmc_traffic.json) is attached only to the workload, kernel and library build it
was measured on and only when its kernel time agrees with its own run's events, and the CPU
baseline runs the reference binary pinned per core without a launcher hop; --dump-outputs writes
the rendered window as float arrays (dump_outputs), and one GPU test runs a plain bench."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_metric_is_baselines():
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert bench.METRIC == base["metric"]


def test_traffic_record_matches_its_build_only():
    rec = json.load(open(os.path.join(REPO, "profiles", "pmc_traffic.json")))
    wl, sha = rec["workload"], rec["lib_sha16"]
    ms = rec["unprofiled_event_ms"]
    got, src = bench.load_traffic(wl, "gss_lin_kernel", ms, sha)
    assert got == rec["hbm_bytes_per_launch"] and "profiled kernel" in src
    # HBM bytes within a few % of the algorithmic bytes: no wasted re-reads
    assert 1.0 <= got / rec["algorithmic_bytes_per_launch"] < 1.05
    assert bench.load_traffic(wl, "gss_lin_kernel", ms, "0" * 16)[0] is None
    assert bench.load_traffic(wl + " x", "gss_lin_kernel", ms, sha)[0] is None
    assert bench.load_traffic(wl, "gss_synth_kernel", ms, sha)[0] is None
    # a run whose kernel time differs from the profile's by more than 10 % gets no traffic
    assert bench.load_traffic(wl, "gss_lin_kernel", ms * 0.8, sha)[0] is None


def test_committed_profile_agrees_with_unprofiled_run():
    """the profile's warm kernel time is within 10 % of the un-profiled run of the same build,
    steps and warm-up (bench.py live_traffic's rule), and not longer than its step"""
    rec = json.load(open(os.path.join(REPO, "profiles", "pmc_traffic.json")))
    prof = rec["kernel_timed_avg_ns"] / 1e6
    assert abs(prof - rec["unprofiled_event_ms"]) <= 0.10 * rec["unprofiled_event_ms"]
    assert rec["steps"] >= 20 and rec["warmup"] >= 5


@pytest.mark.skipif(not os.path.exists(os.path.join(REPO, "oracle", "_ref", "gss_oracle_cli")),
                    reason="oracle not built")
def test_cpu_baseline_short_sample():
    """one process per core of the affinity mask (no cap), plus the 1-core figure"""
    r = bench.cpu_baseline(seconds=1)
    assert r is not None and r["cores"] == len(os.sched_getaffinity(0)) and r["value"] > 0
    assert r["single_core"]["cores"] == 1 and r["kind"] in ("reference", "port")


def test_dtype_label_follows_the_build():
    """bench's dtype names the accumulation the loaded build uses (LIN_MFMA 1 or 2: matrix cores)"""
    sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
    import gpssim_amd as G
    info = G.build_info()
    assert info["lin_mfma"] in ("0", "1", "2")
    assert G.lib_mfma() == (info["lin_mfma"] != "0")
    assert info["lin_mfma"] == "2"                 # the shipped build: channel pairs on MFMA


@pytest.mark.parametrize("fmt,nblk,bb,cap", [(16, 7, 4000, None), (8, 5, 2002, None),
                                              (1, 3, 251, None), (16, 40, 4000, 5 * 2000 + 7),
                                              (8, 9, 300, 2 * 300), (16, 1, 64, None)])
def test_dump_outputs_files(tmp_path, monkeypatch, fmt, nblk, bb, cap):
    """--dump-outputs: checksums over every block, the whole contents of the sampled blocks (all
    of them while they fit, else the first, the last and a seeded choice), float arrays of at
    most 64 MB, the same on every call"""
    import numpy as np
    import torch
    from types import SimpleNamespace
    if cap is not None:                # fewer values than the window holds: a sample
        monkeypatch.setattr(bench, "DUMP_SAMPLE_VALUES", cap)
    raw = np.random.default_rng(fmt + nblk).integers(0, 256, nblk * bb + 5, dtype=np.uint8)
    res = SimpleNamespace(nblk=nblk, bb=bb, out=torch.from_numpy(raw.copy()))
    info = bench.dump_outputs(torch, res, fmt, str(tmp_path / "a"))
    bench.dump_outputs(torch, res, fmt, str(tmp_path / "b"), tag="_rank1")
    got = {n: np.load(tmp_path / "a" / n) for n in info["files"]}
    assert sorted(info["files"]) == sorted(os.listdir(tmp_path / "a"))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) == info["bytes"] <= 64e6
    for n, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / n.replace(".npy", "_rank1.npy")))
    blocks = raw[:nblk * bb].reshape(nblk, bb).astype(np.int64)
    w = np.arange(bb) % 251 + 1
    want = np.stack([blocks.sum(1), (blocks * w).sum(1)], 1)
    assert np.array_equal(got["block_checksums.npy"], want.astype(np.float64))
    idx = got["iq_sample_blocks.npy"].astype(np.int64)
    assert idx[0] == 0 and idx[-1] == nblk - 1 and np.all(np.diff(idx) > 0)
    assert len(idx) == info["sampled_blocks"] == min(nblk, bench.DUMP_SAMPLE_VALUES //
                                                     (bb // 2 if fmt == 16 else bb))
    view = {16: "<i2", 8: "i1", 1: "u1"}[fmt]
    sample = got["iq_sample.npy"]
    assert np.array_equal(sample, raw[:nblk * bb].reshape(nblk, bb)[idx].view(view)
                          .astype(np.float32))


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path, golden):
    """a plain run (no --full) times --steps steps, reports ms_per_step, leaves every other leg
    out, and its --dump-outputs sample holds the reference's blocks (golden block hashes of the
    same static scenario)"""
    import hashlib
    import subprocess
    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--window", "3", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["metric"] == bench.METRIC and d["unit"] == "MS/s" and d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["stages_ms"]["launches_timed"] == 3
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same timing (both rounded to their last printed digit)
    assert abs(d["ms_per_step"] - 29 * 260000 / (d["value"] * 1e3)) <= 0.001
    for leg in ("cpu_baseline", "per_config", "gather", "e2e", "exact_path", "window"):
        assert d[leg] is None, leg
    assert d["stages_ms"]["fast_path_sustained"] is None and d["roofline"]["profile"] is None
    assert sorted(d["dumped_outputs"]["files"]) == sorted(os.listdir(out))
    idx = np.load(out / "iq_sample_blocks.npy").astype(int)
    sample = np.load(out / "iq_sample.npy")
    sums = np.load(out / "block_checksums.npy")
    assert sums.shape == (29, 2) and sample.shape == (len(idx), 2 * 260000) and idx[0] == 0
    want = golden["static_d30_b16"]["block_sha16"]
    for i, b in enumerate(idx):
        raw = sample[i].astype("<i2").tobytes()
        assert hashlib.sha256(raw).hexdigest()[:16] == want[b], b
        assert np.frombuffer(raw, np.uint8).sum() == sums[b, 0]


@pytest.mark.gpu
def test_full_run_caps_the_other_legs_steps():
    """--full with a longer headline (--steps 100, within the library's ring of 256 timed
    launches that launches_timed counts): the headline times all 100, the other legs the
    capped 20 after 5 warm-up steps (here exact_path, window and the sustained launches on a 3 s
    window; the process-starting and long legs off)"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--gpus", "1",
                        "--steps", "100", "--warmup", "7", "--window", "3", "--no-cpu-baseline",
                        "--no-e2e", "--no-configs", "--no-pmc"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["full"] is True and d["steps"] == 100 and d["warmup"] == 7
    assert d["stages_ms"]["launches_timed"] == 100
    assert d["leg_steps"] == bench.LEG_STEPS == 20 and d["leg_warmup"] == bench.LEG_WARMUP == 5
    assert d["exact_path"]["steps"] == 20 and d["exact_path"]["value"] > 0
    assert d["window"]["steps"] == 20 and d["window"]["warmup"] == 5
    assert d["stages_ms"]["fast_path_sustained"] > 0


def test_step_issue_efficiency_bounds():
    """the fast kernel's issue-efficiency line (was roofline_compute) says what it is and carries
    the HBM fraction its step and the formulation's floor allow: 19.6 SIMD
    cycles per wave channel-step at 11.3 channels and 4 B per sample bound the headline at
    ~0.355 of 8 TB/s; the floor and the LDS bound sit above it"""
    r = bench.compute_roofline(8.8e9, 1.466, 4.0, 11.3)
    assert "issue efficiency" in r["what"] and "not an HBM roofline" in r["what"]
    assert abs(r["bound_frac"] - 0.355) < 0.002
    assert r["bound_frac"] < r["floor_bound_frac"] < 1.0
    assert r["bound_frac"] < r["lds_bound_frac"] < 1.0
    # the kernel's HBM fraction over the step's bound = its issue efficiency
    hbm = 8.8e9 / 11.3 * 4.0 / 1.466e-3 / 8e12
    assert abs(hbm / r["bound_frac"] - r["frac"]) < 0.01
    assert "bound_frac" not in bench.compute_roofline(8.8e9, 1.466)    # without the shape
    assert bench.compute_roofline(8.8e9, 0.0) is None
