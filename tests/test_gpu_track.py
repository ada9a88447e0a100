"""Signal tracking on the GPU (csrc/hip/gss_track.hip): Device.track against the numpy restatement
of tests/trk_oracle.py, bit for bit, on both forms of the kernel, on its shapes and on its input
families (epochs of 1 to 135,000 samples on every edge of the fast form's sample loop, saturating
input, the feedback at the ends of its arguments, jobs that end where the samples do); more jobs
than CUs; the state hand-over between launches, also past jobs of no epochs; the scratch
regrowing; and end to end: a noisy run of the synthesiser
is tracked on the device for 12.4 s, and the subframes read back are its nav rows' words at the
samples its channel rows say."""
import subprocess

import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import acq_oracle as A
import trk_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
PATHS = ["fast", "plain"]


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def set_path(monkeypatch, path, chunk=None):
    if path == "plain":
        monkeypatch.setenv("GSS_TRK_PATH", "plain")
    else:
        monkeypatch.delenv("GSS_TRK_PATH", raising=False)
    if chunk:
        monkeypatch.setenv("GSS_TRK_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("GSS_TRK_CHUNK", raising=False)


def on_device(dev, trk, data, N, jobs, pitch, in_off=0):
    """Device.track over data placed in_off bytes into a device buffer; the records and counts
    sit between 0xA5 guard bytes, which must survive, and records past a job's count must stay
    untouched: (rec [n_job, pitch], count)"""
    import torch
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    d_in = torch.zeros(len(data) + in_off + 16, dtype=torch.uint8, device="cuda")
    d_in[in_off:in_off + len(data)] = torch.from_numpy(data.copy()).cuda()
    sizes = [64 * len(jobs) * pitch, 4 * len(jobs)]
    bufs = [torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            for n in sizes]
    ptr = [b.data_ptr() + GUARD for b in bufs]
    assert all(p % 8 == 0 for p in ptr)
    dev.track(trk, d_in.data_ptr() + in_off, N, jobs, ptr[0], pitch, ptr[1])
    torch.cuda.synchronize()
    outs = []
    for b, n in zip(bufs, sizes):
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), "wrote outside"
        outs.append(h[GUARD:GUARD + n].copy())
    rec = outs[0].view(G.TRK_REC_DTYPE).reshape(len(jobs), pitch)
    count = outs[1].view(np.int32)
    raw = outs[0].reshape(len(jobs), pitch * 64)
    for j, c in enumerate(count):
        assert 0 <= c <= pitch and (raw[j, 64 * c:] == 0xA5).all(), ("wrote past its count", j)
    return rec, count


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("si", range(len(O.SHAPES)))
def test_device_equals_oracle(dev, monkeypatch, si, fmt, path):
    fs, N, n_pull, jobs = O.SHAPES[si]
    data, wrec, wcount = O.want(si, fmt, 10 * si + fmt)
    set_path(monkeypatch, path)
    rec, count = on_device(dev, O.trk_of(fs, fmt, O.gains_of(fs, n_pull)), data, N,
                           O.jobs_array(jobs), wrec.shape[1], in_off=2 if fmt == 16 else 1)
    O.same_records(rec, count, wrec, wcount)


def device_equals(dev, c, in_off=0):
    rec, count = on_device(dev, O.trk_of(c["fs"], c["fmt"], c["gains"]), c["data"], c["N"],
                           O.jobs_array(c["jobs"]), c["pitch"], in_off=in_off)
    O.same_records(rec, count, c["rec"], c["count"])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", O.RATES)
def test_device_at_every_length(dev, monkeypatch, name, path):
    """epochs of 1 to 135,000 samples: each edge of the fast form's sample loop (the samples
    loaded ahead, the passes of four behind them, the flush of the int32 sums)"""
    c = O.case(name)
    set_path(monkeypatch, path)
    device_equals(dev, c, in_off=2 if c["fmt"] == 16 else 1)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", O.SATURATING)
def test_device_saturating(dev, monkeypatch, name, path):
    """a lane's prompt sum passes 2^31 within the epoch: wrong without the flush into int64"""
    set_path(monkeypatch, path)
    device_equals(dev, O.case(name))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", O.FEEDBACK + O.ENDS)
def test_device_feedback_and_ends(dev, monkeypatch, name, path):
    set_path(monkeypatch, path)
    device_equals(dev, O.case(name))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunk", [1, 7, 40])
def test_hand_over_with_jobs_that_end_early(dev, monkeypatch, chunk, path):
    """Launches of 1, 7 and all 40 epochs over jobs of 0, 1 and 40 epochs, one of which ends
    one sample short of its 40th and one runs out of samples in its eleventh (the second launch
    of 7).  Jobs finish in different launches; the job of no epochs, whose state only the first
    launch can write, keeps count 0 and untouched records through every later one."""
    c = O.case("ends_64000_short")
    assert list(c["count"]) == [39, 0, 0, 0, 0, 1, 10] and c["jobs"][4][3] == 0
    assert max(j[3] for j in c["jobs"]) == 40
    set_path(monkeypatch, path, chunk=chunk)
    device_equals(dev, c)


@pytest.mark.parametrize("path", PATHS)
def test_state_hand_over_between_launches(dev, monkeypatch, path):
    """60 epochs in launches of 16: the state written back by one launch continues the next"""
    fs, N, n_pull, jobs = O.SHAPES[0]
    data, wrec, wcount = O.want(0, 16, 16)
    set_path(monkeypatch, path, chunk=16)
    rec, count = on_device(dev, O.trk_of(fs, 16, O.gains_of(fs, n_pull)), data, N,
                           O.jobs_array(jobs), wrec.shape[1])
    O.same_records(rec, count, wrec, wcount)


def many_jobs(n_job=300, fs=64000, ne=12):
    """more workgroups than CUs, each an epoch of one wave: (data, N, jobs, gains, rec, count)"""
    if "many" not in O._want:
        N = (ne + 6) * 64
        rng = np.random.default_rng(77)
        jobs = [(int(rng.integers(1, 33)), int(rng.integers(0, 5 * 64)),
                 O._w(int(rng.integers(-5000, 5001)), fs), ne - j % 3) for j in range(n_job)]
        data = O.random_samples(N, 16, 78)
        gains = O.gains_of(fs, 5)
        O._want["many"] = (data, N, jobs, gains) + O.track(data, 16, N, fs, gains, jobs, ne)
    return O._want["many"]


@pytest.mark.parametrize("path", PATHS)
def test_more_jobs_than_cus(dev, monkeypatch, path):
    data, N, jobs, gains, wrec, wcount = many_jobs()
    set_path(monkeypatch, path)
    rec, count = on_device(dev, O.trk_of(64000, 16, gains), data, N, O.jobs_array(jobs),
                           wrec.shape[1], in_off=2)
    O.same_records(rec, count, wrec, wcount)


def test_scratch_regrows(dev, monkeypatch):
    """a small call, then one with more jobs than any before on this handle, then small again"""
    set_path(monkeypatch, "fast")
    fs, N, n_pull, jobs = O.SHAPES[0]
    data, wrec, wcount = O.want(0, 16, 16)
    trk = O.trk_of(fs, 16, O.gains_of(fs, n_pull))
    rec, count = on_device(dev, trk, data, N, O.jobs_array(jobs[:1]), wrec.shape[1])
    O.same_records(rec, count, wrec[:1], wcount[:1])
    mdata, mN, mjobs, gains, mrec, mcount = many_jobs()
    big = mjobs + mjobs[:100]
    rec, count = on_device(dev, O.trk_of(64000, 16, gains), mdata, mN, O.jobs_array(big),
                           mrec.shape[1])
    O.same_records(rec, count, np.concatenate([mrec, mrec[:100]]),
                   np.concatenate([mcount, mcount[:100]]))
    rec, count = on_device(dev, trk, data, N, O.jobs_array(jobs), wrec.shape[1])
    O.same_records(rec, count, wrec, wcount)


def test_each_handle_owns_its_scratch(monkeypatch):
    """Calls alternate between handles of one device, one job and 400, and go on after a handle
    is closed and on a handle opened afterwards.  Every call leaves its state in its handle's own
    state buffer, and in launches of 16 epochs the calls of 60 epochs continue from it: a buffer
    shared between handles, or one that survived a close, would show in the records."""
    set_path(monkeypatch, "fast", chunk=16)
    fs, N, n_pull, jobs = O.SHAPES[0]
    data, wrec, wcount = O.want(0, 16, 16)
    trk = O.trk_of(fs, 16, O.gains_of(fs, n_pull))
    mdata, mN, mjobs, gains, mrec, mcount = many_jobs()

    def small(d):
        rec, count = on_device(d, trk, data, N, O.jobs_array(jobs[:1]), wrec.shape[1])
        O.same_records(rec, count, wrec[:1], wcount[:1])

    def large(d):
        rec, count = on_device(d, O.trk_of(64000, 16, gains), mdata, mN,
                               O.jobs_array(mjobs + mjobs[:100]), mrec.shape[1])
        O.same_records(rec, count, np.concatenate([mrec, mrec[:100]]),
                       np.concatenate([mcount, mcount[:100]]))

    open_handles = []

    def opened():
        open_handles.append(G.Device(0))
        return open_handles[-1]

    try:
        a = opened()
        small(a)
        b = opened()
        large(b)
        small(a)
        a.close()
        small(b)
        b.close()
        c = opened()
        large(c)
    finally:
        for d in open_handles:
            d.close()


def test_device_argument_errors(dev):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok, okj = G.Trk(64000, 16), O.jobs_array([(1, 0, 0, 4)])
    low = G.Trk(64000, 16)
    low.fs_hz = 1000
    for trk, jobs, x, r, c, pitch in [
            (ok, O.jobs_array([(33, 0, 0, 4)]), p, p + 4096, p + 8192, 4),
            (ok, O.jobs_array([(1, -5, 0, 4)]), p, p + 4096, p + 8192, 4),
            (ok, O.jobs_array([(1, 2**63 - 1, 0, 4)]), p, p + 4096, p + 8192, 4),
            (ok, O.jobs_array([(1, 2**62 + 1, 0, 4)]), p, p + 4096, p + 8192, 4),
            (ok, okj, p, p + 4096, p + 8192, 3),
            (low, okj, p, p + 4096, p + 8192, 4),
            (G.Trk(64000, 16, Ki=-1), okj, p, p + 4096, p + 8192, 4),
            (ok, okj, p + 1, p + 4096, p + 8192, 4), (ok, okj, p, p + 4097, p + 8192, 4),
            (ok, okj, p, p + 4096, p + 8193, 4), (ok, okj, 0, p + 4096, p + 8192, 4),
            (ok, okj, p, 0, p + 8192, 4), (ok, okj, p, p + 4096, 0, 4)]:
        with pytest.raises(G.GssError) as e:
            dev.track(trk, x, 1000, jobs, r, pitch, c)
        assert e.value.code == -1
    # A code step that could fall to M >> 23 (an epoch of 2^23 samples and more) is refused by
    # the argument check, which runs before any launch; just inside the bound the call runs,
    # and the one epoch, longer than the samples, does not.
    far = O.jobs_array([(1, 0, -2**31, 4)])
    fs, inside, outside = O.longest_cfg()
    x8 = O.random_samples(1000, 8, 2)
    for trk in (G.Trk(fs, 8, n_pull=0, Kf=0, Ki=0, Kp=0, Kd=3209600), O.trk_of(fs, 8, outside)):
        with pytest.raises(G.GssError) as e:
            dev.track(trk, p, 1000, far, p + 4096, 4, p + 8192)
        assert e.value.code == -1
        with pytest.raises(G.GssError) as e:
            dev.track_from_host(trk, x8, far)
        assert e.value.code == -1
    rec, count = on_device(dev, O.trk_of(fs, 8, inside), x8, 1000, far, 4)
    assert count[0] == 0
    torch.cuda.synchronize()


def test_from_host_buffers(dev, monkeypatch):
    set_path(monkeypatch, "fast")
    fs, N, n_pull, jobs = O.SHAPES[1]
    data, wrec, wcount = O.want(1, 8, 18)
    rec, count = dev.track_from_host(O.trk_of(fs, 8, O.gains_of(fs, n_pull)), data,
                                     O.jobs_array(jobs), n=N)
    O.same_records(rec, count, wrec, wcount)


_runs = {}


def noisy_run(dev, fmt):
    """the bytes of the physical run (125 blocks, noise at PHYS_CN0, seed 7) from gss_run"""
    if fmt not in _runs:
        imp = G.Impair(O.phys_sigma(), 2 if fmt == 8 else 0, 7)
        s = G.Scenario(NAV, llh=LOC, duration=O.PHYS_DURATION, samp_freq=float(A.PHYS_FS),
                       data_format=fmt)
        parts = []
        dev.run(s, lambda buf, b0, nb: parts.append(np.frombuffer(bytes(buf), np.uint8)),
                n_blocks=O.PHYS_BLOCKS, batch=25, impair=imp)
        s.close()
        _runs[fmt] = np.concatenate(parts)
        assert len(_runs[fmt]) == O.PHYS_BLOCKS * G.block_bytes(100000, fmt)
    return _runs[fmt]


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_end_to_end(dev, monkeypatch, fmt):
    """gss_run with noise, its whole output uploaded again and tracked on the device: the host's
    records, and every steady satellite's subframes are its nav rows' words where its channel
    rows put them (fails if the synthesiser's bit edges, parity words or Doppler sign ever drift
    from its rows)"""
    set_path(monkeypatch, "fast")
    data = noisy_run(dev, fmt)
    acq = O.phys_acq(fmt)
    peaks, _, _ = dev.acquire_from_host(acq, data[:acq.sample_bytes()])
    jobs, keep = O.phys_jobs(fmt, peaks)
    assert len(jobs) == len(keep) >= 8
    trk = G.Trk(A.PHYS_FS, fmt)
    N = O.PHYS_BLOCKS * 100000
    rec, count = on_device(dev, trk, data, N, jobs, O.PHYS_EPOCHS)
    hrec, hcount = G.track_host(trk, data, jobs, n=N, threads=8)
    O.same_records(rec, count, hrec, hcount)
    O.check_decode(rec, count, jobs, keep, level=O.LEVEL if fmt != 1 else None)


def test_tool_on_the_gpu(dev, tmp_path):
    """gps-sdr-track without --host prints what --host prints, and writes the same records"""
    f = tmp_path / "run.bin"
    noisy_run(dev, 16).tofile(f)
    args = [G.TRK_CLI_PATH, "-f", str(f), "-s", str(A.PHYS_FS), "--prn=1,4,6,17,28"]
    gpu = subprocess.run(args + [f"--records={tmp_path / 'g.bin'}"], capture_output=True,
                         text=True)
    host = subprocess.run(args + ["--host", f"--records={tmp_path / 'h.bin'}"],
                          capture_output=True, text=True)
    assert gpu.returncode == 0 and host.returncode == 0, gpu.stderr + host.stderr
    assert gpu.stdout == host.stdout
    lines = gpu.stdout.splitlines()
    assert [ln.split()[1] for ln in lines if ln.startswith("PRN")] == ["1", "6", "17", "28"]
    assert sum(ln.startswith("SF") for ln in lines) >= 4
    assert (tmp_path / "g.bin").read_bytes() == (tmp_path / "h.bin").read_bytes()
    # three windows of the four strongest satellites (45 dB-Hz and more: found in every window)
    args = args[:-1] + ["--prn=6,10,17,28", "--split=1.0", "-d", "3.0"]
    split = subprocess.run(args, capture_output=True, text=True)
    hsplit = subprocess.run(args + ["--host"], capture_output=True, text=True)
    assert split.returncode == 0 and split.stdout == hsplit.stdout
    heads = [ln.split() for ln in split.stdout.splitlines() if ln.startswith("PRN")]
    assert [(int(h[3]), int(h[1])) for h in heads] == [(w, p) for w in range(3)
                                                      for p in (6, 10, 17, 28)]
    assert all(int(h[7]) == 1 for h in heads)
