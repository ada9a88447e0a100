"""Observables on the GPU (csrc/hip/gss_obs.hip) and fixes from device-side records:
Device.observables against the restatement of tests/obs_oracle.py, byte for byte, on both forms
of the kernel and on every shape of the CPU tests (counts on every edge of the kernel's scan, a
job of 70,000 records beside 299 of three, more jobs than CUs), between guard bytes and at a
record's offset; and end to end: a noisy run of the synthesiser is searched, tracked and
measured with its records left on the device, and the fixes come out at the scenario's location
and start time, also with navigation data from the decoded subframes alone, and on the circle's
path."""
import numpy as np
import pytest

from conftest import CIRCLE, LOC, NAV

import gpssim_amd as G
import acq_oracle as A
import obs_oracle as B
import trk_oracle as O
import test_pvt as P

pytestmark = pytest.mark.gpu

GUARD = 64
PATHS = ["fast", "plain"]


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def set_path(monkeypatch, path):
    if path == "plain":
        monkeypatch.setenv("GSS_OBS_PATH", "plain")
    else:
        monkeypatch.delenv("GSS_OBS_PATH", raising=False)


def on_device(dev, fs, rec, count, grid, rec_off=0):
    """Device.observables over records placed rec_off bytes into a device buffer; the
    observables sit between 0xA5 guard bytes, which must survive: obs [n_job, n_fix]"""
    import torch
    n_job, pitch = rec.shape
    n_fix = grid[2]
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)
    d_rec = torch.zeros(len(raw) + rec_off + 64, dtype=torch.uint8, device="cuda")
    if len(raw):
        d_rec[rec_off:rec_off + len(raw)] = torch.from_numpy(raw.copy()).cuda()
    d_count = torch.from_numpy(np.ascontiguousarray(count, np.int32).copy()).cuda()
    n = 32 * n_job * n_fix
    d_obs = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dev.observables(fs, d_rec.data_ptr() + rec_off, pitch, d_count.data_ptr(), n_job, *grid,
                    d_obs.data_ptr() + GUARD)
    torch.cuda.synchronize()
    h = d_obs.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), "wrote outside"
    return h[GUARD:GUARD + n].copy().view(G.OBS_DTYPE).reshape(n_job, n_fix)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", B.NAMES)
def test_device_equals_oracle(dev, monkeypatch, name, path):
    set_path(monkeypatch, path)
    c = B.case(name)
    for g, grid in enumerate(c["grids"]):
        B.same(on_device(dev, c["fs"], c["rec"], c["count"], grid), B.want(name, g))


@pytest.mark.parametrize("path", PATHS)
def test_records_at_an_offset(dev, monkeypatch, path):
    """d_rec one record into its allocation (64 bytes: 8-byte aligned is all the call asks)"""
    set_path(monkeypatch, path)
    for name in ("edges", "small"):
        c = B.case(name)
        B.same(on_device(dev, c["fs"], c["rec"], c["count"], c["grids"][0], rec_off=64),
               B.want(name, 0))
        B.same(on_device(dev, c["fs"], c["rec"], c["count"], c["grids"][1], rec_off=8),
               B.want(name, 1))


def test_one_job_then_many_then_one(dev, monkeypatch):
    """1 job, 400 and 1 again on one handle (the kernel keeps no scratch: nothing may depend on
    an earlier call's size)"""
    set_path(monkeypatch, "fast")
    c, big = B.case("small"), B.case("big")
    one = lambda: B.same(on_device(dev, c["fs"], c["rec"][3:], c["count"][3:], c["grids"][3]),
                         B.want("small", 3)[3:])
    one()
    rec = np.concatenate([big["rec"], big["rec"][:100]])
    count = np.concatenate([big["count"], big["count"][:100]])
    assert len(count) == 400
    w = B.want("big", 0)
    B.same(on_device(dev, big["fs"], rec, count, big["grids"][0]), np.concatenate([w, w[:100]]))
    one()


def test_from_host_buffers_and_arguments(dev, monkeypatch):
    import torch
    set_path(monkeypatch, "fast")
    c = B.case("edges")
    B.same(dev.observables_from_host(c["fs"], c["rec"], c["count"], *c["grids"][0]),
           B.want("edges", 0))
    buf = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for args in [(4000, p, 4, p + 1024, 1, 0, 0, 2, p + 2048), (999, p, 4, p + 1024, 1, 0, 1, 2, p + 2048),
                 (4000, p + 4, 4, p + 1024, 1, 0, 1, 2, p + 2048), (4000, p, 4, p + 1025, 1, 0, 1, 2, p + 2048),
                 (4000, p, 4, p + 1024, 1, 0, 1, 2, p + 2052), (4000, p, 4, 0, 1, 0, 1, 2, p + 2048),
                 (4000, p, 4, p + 1024, 1, 0, 1, 2, 0), (4000, p, 4, p + 1024, 0, 0, 1, 2, p + 2048)]:
        with pytest.raises(G.GssError) as e:
            dev.observables(*args)
        assert e.value.code == -1
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------
def run_bytes(dev, fmt, n_blocks, sigma, **where):
    """(the bytes of gss_run over n_blocks blocks at 1 MS/s, the rows' steady channels)"""
    s = G.Scenario(NAV, duration=n_blocks / 10 + 0.1, samp_freq=float(A.PHYS_FS), data_format=fmt,
                   **where)
    parts = []
    dev.run(s, lambda buf, b0, nb: parts.append(np.frombuffer(bytes(buf), np.uint8)),
            n_blocks=n_blocks, batch=25,
            impair=G.Impair(sigma, 2 if fmt == 8 and sigma else 0, 7) if sigma else None)
    s.close()
    s = G.Scenario(NAV, duration=n_blocks / 10 + 0.1, samp_freq=float(A.PHYS_FS), **where)
    blk, nch = s.next(n_blocks)
    s.close()
    assert len(nch) == n_blocks
    return np.concatenate(parts), O.steady_channels(blk, nch)


def device_chain(dev, fmt, data, keep, n_epoch):
    """search, Device.track and Device.observables with the records left on the device:
    (rec, count, jobs, obs, grid), the records downloaded afterwards"""
    import torch
    fs = A.PHYS_FS
    acq = O.phys_acq(fmt)
    peaks, _, _ = dev.acquire_from_host(acq, data[:acq.sample_bytes()])
    sel = np.array([p for p in peaks if int(p["prn"]) in keep], G.ACQ_PEAK_DTYPE)
    jobs = G.trk_jobs(acq, sel, 0, n_epoch)
    assert len(jobs) == len(keep) >= 8
    N = {16: len(data) // 4, 8: len(data) // 2, 1: len(data) * 4}[fmt]
    d_in = torch.from_numpy(data.copy()).cuda()
    d_rec = torch.zeros(64 * len(jobs) * n_epoch, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(len(jobs), dtype=torch.int32, device="cuda")
    dev.track(G.Trk(fs, fmt), d_in.data_ptr(), N, jobs, d_rec.data_ptr(), n_epoch,
              d_count.data_ptr())
    # the grid needs the records' samples only to skip the pull-in: every job is past epoch
    # FIRST_EPOCH a code period and the search's offset after FIRST_EPOCH ms
    step = fs // P.RATE_HZ
    k0 = -(-(P.FIRST_EPOCH + 2) * 1000 // step)
    n_fix = (n_epoch - 2) * 1000 // step - k0
    grid = (k0 * step, step, n_fix)
    d_obs = torch.zeros(32 * len(jobs) * n_fix, dtype=torch.uint8, device="cuda")
    dev.observables(fs, d_rec.data_ptr(), n_epoch, d_count.data_ptr(), len(jobs), *grid,
                    d_obs.data_ptr())
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy().view(G.TRK_REC_DTYPE).reshape(len(jobs), n_epoch)
    count = d_count.cpu().numpy()
    obs = d_obs.cpu().numpy().view(G.OBS_DTYPE).reshape(len(jobs), n_fix)
    assert (count == n_epoch).all()
    B.same(obs, G.observables_host(fs, rec, count, *grid))
    assert (obs["epoch"] >= P.FIRST_EPOCH).all()
    return rec, count, jobs, obs, grid


def bounds(run):
    md, mdt, mv, _ = P.MEASURED[run]
    return min(2 * md, P.CAP_M), min(2 * mdt * 1e-9, P.CAP_S), 2 * mv


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_end_to_end(dev, monkeypatch, fmt):
    """gss_run with noise, its output uploaded again, searched, tracked and measured on the
    device: the observables are the host's on the downloaded records, and the fixes meet the CPU
    test's bounds"""
    set_path(monkeypatch, "fast")
    data, keep = run_bytes(dev, fmt, O.PHYS_BLOCKS, O.phys_sigma(), llh=LOC)
    rec, count, jobs, obs, grid = device_chain(dev, fmt, data, keep, O.PHYS_EPOCHS)
    nd = G.NavData(NAV)
    fixes = P.fixes_of(nd, float(A.PHYS_FS), rec, count, jobs, obs, grid)
    nd.close()
    d, dt, v = P.worst_of(fixes, P.start_time(), P.llh_to_ecef(*LOC))
    print(fmt, "distance", d, "m, |T0 - g0|", dt * 1e9, "ns, speed", v, "m/s,", len(fixes), "fixes")
    bd, bdt, bv = bounds(f"sc{fmt:02d}")
    assert len(fixes) >= 100 and d <= bd and dt <= bdt and v <= bv


def test_unassisted(dev, monkeypatch):
    """40 s noise-free, navigation data from the decoded subframes alone (subframes 2 and 3 of
    the first frame, 1 of the second, page 18): fixes within the noise-free bounds"""
    set_path(monkeypatch, "fast")
    data, keep = run_bytes(dev, 16, 400, 0, llh=LOC)
    rec, count, jobs, obs, grid = device_chain(dev, 16, data, keep, 39900)
    nd = G.NavData()
    g0 = P.start_time()
    fixes = P.fixes_of(nd, float(A.PHYS_FS), rec, count, jobs, obs, grid, week=g0[0])
    assert all(nd.get(int(j["prn"]))["valid"] == 1 for j in jobs)
    assert nd.get(int(jobs[0]["prn"]))["iono_valid"] == 1
    nd.close()
    d, dt, v = P.worst_of(fixes, g0, P.llh_to_ecef(*LOC))
    print("unassisted distance", d, "m, |T0 - g0|", dt * 1e9, "ns, speed", v, "m/s,", len(fixes),
          "fixes")
    bd, bdt, bv = bounds("clean16")
    assert len(fixes) >= 380 and d <= bd and dt <= bdt and v <= bv


def test_moving_receiver(dev, monkeypatch):
    """the circle's path, 12.5 s with noise on SC16: fix k lies within the position bound of row
    k of the motion file (instants at multiples of 0.1 s from sample 0)"""
    set_path(monkeypatch, "fast")
    data, keep = run_bytes(dev, 16, O.PHYS_BLOCKS, O.phys_sigma(), motion_file=CIRCLE)
    rec, count, jobs, obs, grid = device_chain(dev, 16, data, keep, O.PHYS_EPOCHS)
    path = np.loadtxt(CIRCLE, delimiter=",")[:, 1:4]
    nd = G.NavData(NAV)
    fixes = P.fixes_of(nd, float(A.PHYS_FS), rec, count, jobs, obs, grid)
    nd.close()
    assert all(f.status == G.PVT_OK for f in fixes)
    k0 = grid[0] // grid[1]
    err = [float(np.linalg.norm(np.array(f.xyz) - path[k0 + k])) for k, f in enumerate(fixes)]
    print("moving: worst distance", max(err), "m over", len(err), "fixes")
    assert len(err) >= 100 and max(err) <= bounds("sc16")[0]


def test_tool_on_the_gpu(dev, tmp_path):
    """gps-sdr-pvt without --host prints what --host prints, and writes the same csv"""
    import subprocess
    data, keep = run_bytes(dev, 16, O.PHYS_BLOCKS, O.phys_sigma(), llh=LOC)
    f = tmp_path / "run.bin"
    data.tofile(f)
    args = [G.PVT_CLI_PATH, "-f", str(f), "-s", str(A.PHYS_FS), "-e", NAV, "--prn=1,4,6,10,17,28"]
    gpu = subprocess.run(args + [f"--csv={tmp_path / 'g.csv'}"], capture_output=True, text=True)
    host = subprocess.run(args + ["--host", f"--csv={tmp_path / 'h.csv'}"], capture_output=True,
                          text=True)
    assert gpu.returncode == 0 and host.returncode == 0, gpu.stderr + host.stderr
    assert gpu.stdout == host.stdout and gpu.stderr == host.stderr
    fixes = P.tool_fixes(gpu.stdout)
    assert len(fixes) >= 100 and all(f["sats"] >= 4 for f in fixes.values())
    xyz = P.llh_to_ecef(*LOC)
    assert max(np.linalg.norm(np.array(f["xyz"]) - xyz) for f in fixes.values()) < P.CAP_M
    assert (tmp_path / "g.csv").read_bytes() == (tmp_path / "h.csv").read_bytes()
