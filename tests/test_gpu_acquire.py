"""The acquisition search on the GPU (csrc/hip/gss_acquire.hip): Device.acquire against the numpy
restatement of tests/acq_oracle.py, bit for bit, on the matrix-core path and the VALU path, at
the oracle's edge shapes (odd window lengths, tile and chunk edges), planted peaks and ties too;
the scratch regrowing between calls; and end to end: a noisy run's first block holds the satellites
its channel rows describe, at the level the noise option asked for."""
import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import acq_oracle as O
from acq_oracle import SHAPES, random_samples

pytestmark = pytest.mark.gpu

BIG = (1000000, 1, 8, 10, 500, tuple(range(1, 33)))       # the physical test's search
LARGE = (2600000, 1, 2, 2, 500, (3, 30))                  # larger than every shape of SHAPES
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def on_device(dev, acq, data, in_off=0, want_grid=True):
    """Device.acquire over data placed in_off bytes into a device buffer; the outputs sit between
    0xA5 guard bytes, which must survive: (peaks, grid or None, resolved shift)"""
    import torch
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    _, T, _, _, P = acq.sizes()
    nb = acq.sample_bytes()
    d_in = torch.zeros(nb + in_off + 16, dtype=torch.uint8, device="cuda")
    d_in[in_off:in_off + nb] = torch.from_numpy(data[:nb].copy()).cuda()
    sizes = [32 * P, 8 * P * (2 * acq.n_half + 1) * T if want_grid else 0, 4]
    bufs = [torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            for n in sizes]
    ptr = [b.data_ptr() + GUARD for b in bufs]
    assert all(p % 8 == 0 for p in ptr)
    dev.acquire(acq, d_in.data_ptr() + in_off, ptr[0], ptr[1] if want_grid else 0, ptr[2])
    torch.cuda.synchronize()
    outs = []
    for b, n in zip(bufs, sizes):
        h = b.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), "wrote outside"
        outs.append(h[GUARD:GUARD + n].copy())
    peaks = outs[0].view(G.ACQ_PEAK_DTYPE)
    grid = outs[1].view(np.uint64).reshape(P, 2 * acq.n_half + 1, T) if want_grid else None
    return peaks, grid, int(outs[2].view(np.int32)[0])


def acq_of(shape, fmt=16, qshift=-1):
    fs, coh, M, K, df, prns = shape
    return G.Acq(fs, fmt, coh, M, df, K, qshift, prns)


_want = {}


def want(key, shape, fmt, data, qshift):
    """the oracle's answer, computed once per input and shared by both paths"""
    if key not in _want:
        fs, coh, M, K, df, prns = shape
        _want[key] = O.acquire(data, fs, fmt, coh, M, K, df, prns, qshift)
    return _want[key]


def cases():
    out = []
    for si, s in enumerate(SHAPES):
        for q in (0, 7, -1):
            out.append((f"s{si}-q{q}", s, 16, ("rand", si + 1), q))
        out.append((f"s{si}-extreme", s, 16, ("extreme", 50 + si), -1))
    for si in (0, 1):
        for fmt in (8, 1):
            out.append((f"s{si}-b{fmt}", SHAPES[si], fmt, ("rand", 20 + si), -1))
    out.append(("big", BIG, 16, ("rand", 99), -1))
    return out + O.edge_cases() + O.SPECIAL_CASES


CASES = cases()


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_oracle(dev, monkeypatch, case, path):
    name, shape, fmt, _, qshift = case
    data = O.case_data(case)
    wp, wg, wsh = O.answer(case)
    if path == "valu":
        monkeypatch.setenv("GSS_ACQ_PATH", "valu")
    else:
        monkeypatch.delenv("GSS_ACQ_PATH", raising=False)
    acq = acq_of(shape, fmt, qshift)
    peaks, grid, sh = on_device(dev, acq, data, in_off=2 if fmt == 16 else 1)
    assert sh == wsh
    assert np.array_equal(grid, wg), np.argwhere(grid != wg)[:8]
    assert np.array_equal(peaks, wp)
    peaks, none, sh = on_device(dev, acq, data, in_off=6 if fmt == 16 else 3, want_grid=False)
    assert sh == wsh and np.array_equal(peaks, wp)


@pytest.mark.parametrize("path", ["mfma", "valu"])
def test_scratch_regrows(dev, monkeypatch, path):
    """two searches on one handle, the second larger in every scratch buffer than any before"""
    if path == "valu":
        monkeypatch.setenv("GSS_ACQ_PATH", "valu")
    small = SHAPES[0]
    large = LARGE[:2] + (2 + (path == "valu"),) + LARGE[3:]
    for tag, s in (("small", small), ("large", large)):
        data = random_samples(s[0], s[1], s[2], 16, seed=7)
        wp, wg, wsh = want(("regrow", s), s, 16, data, -1)
        peaks, none, sh = on_device(dev, acq_of(s), data, want_grid=False)
        assert sh == wsh and np.array_equal(peaks, wp), tag
        peaks, grid, sh = on_device(dev, acq_of(s), data)
        assert np.array_equal(grid, wg) and np.array_equal(peaks, wp), tag


def edge_case(si, tag="q-1"):
    return next(c for c in O.edge_cases() if c[0] == f"e{si}-{tag}")


@pytest.mark.parametrize("path", ["mfma", "valu"])
def test_scratch_regrows_at_odd_lengths(monkeypatch, path):
    """a new handle goes from L = 65 to L = 1023 to L = 4095: the padded plane and replica
    lengths grow while the windows start off a dword boundary"""
    if path == "valu":
        monkeypatch.setenv("GSS_ACQ_PATH", "valu")
    else:
        monkeypatch.delenv("GSS_ACQ_PATH", raising=False)
    d = G.Device(0)
    try:
        for si in (0, 1, 6):
            case = edge_case(si)
            wp, wg, wsh = O.answer(case)
            data = O.case_data(case)
            peaks, none, sh = on_device(d, acq_of(case[1]), data, want_grid=False)
            assert sh == wsh and np.array_equal(peaks, wp), si
            peaks, grid, sh = on_device(d, acq_of(case[1]), data)
            assert np.array_equal(grid, wg) and np.array_equal(peaks, wp), si
    finally:
        d.close()


def test_each_handle_owns_its_scratch(monkeypatch):
    """Searches alternate between handles of one device, small and large, and go on after a
    handle is closed and on a handle opened afterwards: a capacity or a pointer shared between
    handles, or one that survived a close, would show as a wrong grid or a fault."""
    monkeypatch.delenv("GSS_ACQ_PATH", raising=False)

    def run(d, s, want_grid):
        data = random_samples(s[0], s[1], s[2], 16, seed=7)
        wp, wg, wsh = want(("regrow", s), s, 16, data, -1)
        peaks, grid, sh = on_device(d, acq_of(s), data, want_grid=want_grid)
        assert sh == wsh and np.array_equal(peaks, wp)
        assert not want_grid or np.array_equal(grid, wg)

    open_handles = []

    def opened():
        open_handles.append(G.Device(0))
        return open_handles[-1]

    try:
        a = opened()
        run(a, SHAPES[0], False)
        b = opened()
        run(b, LARGE, True)
        run(a, SHAPES[0], True)
        a.close()
        run(b, SHAPES[0], True)
        b.close()
        c = opened()
        run(c, LARGE, True)
    finally:
        for d in open_handles:
            d.close()


def test_device_argument_errors(dev):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = G.Acq(64000, 16, 1, 1, 500, 1, -1, [1])
    for acq, x, pk in [(G.Acq(64000, 16, 1, 1001, 500, 1, -1, [1]), p, p + 4096),
                       (G.Acq(4000, 16, 1, 1, 500, 1, -1, [1]), p, p + 4096),
                       (ok, p + 1, p + 4096), (ok, p, p + 4097), (ok, 0, p + 4096), (ok, p, 0)]:
        with pytest.raises(G.GssError) as e:
            dev.acquire(acq, x, pk)
        assert e.value.code == -1
    torch.cuda.synchronize()


def test_from_host_buffers(dev):
    s = SHAPES[1]
    data = random_samples(s[0], s[1], s[2], 16, seed=2)
    wp, wg, wsh = O.acquire(data, s[0], 16, s[1], s[2], s[3], s[4], s[5], -1)
    peaks, grid, sh = dev.acquire_from_host(acq_of(s), data, want_grid=True)
    assert sh == wsh and np.array_equal(grid, wg) and np.array_equal(peaks, wp)


def test_from_host_buffers_odd_length(dev, monkeypatch):
    """gss_acquire's own upload and download at L = T = 1023 with 17 PRNs"""
    monkeypatch.delenv("GSS_ACQ_PATH", raising=False)
    case = edge_case(1)
    wp, wg, wsh = O.answer(case)
    peaks, grid, sh = dev.acquire_from_host(acq_of(case[1]), O.case_data(case), want_grid=True)
    assert sh == wsh and np.array_equal(grid, wg) and np.array_equal(peaks, wp)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_end_to_end(dev, fmt):
    """gss_run with noise at 50 dB-Hz, the search over the run's first block on the device: the
    host's peaks, and the satellites where the rows say (fails if the synthesiser's code phase,
    Doppler sign or noise level ever drifts from its rows)"""
    fs = O.PHYS_FS
    sigma = int(np.floor(256 * 250 * np.sqrt(fs / (2 * 10 ** (O.PHYS_CN0 / 10))) + 0.5))
    imp = G.Impair(sigma, 2 if fmt == 8 else 0, 7)
    s = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(fs), data_format=fmt)
    bb = G.block_bytes(s.n_per_blk, fmt)
    first = []

    def sink(buf, b0, nb):
        if b0 == 0:
            first.append(np.frombuffer(bytes(buf[:bb]), np.uint8))

    dev.run(s, sink, batch=4, impair=imp)
    s.close()
    rows = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(fs))
    blk, nch = rows.next(1)
    rows.close()
    acq = O.PHYS_ACQ(fmt)
    peaks, _, sh = on_device(dev, acq, first[0], want_grid=False)
    hp, _, hsh = G.acquire_host(acq, first[0])
    assert sh == hsh and np.array_equal(peaks, hp)
    O.check_physical(peaks, blk, nch, level=fmt != 1, found=fmt != 1)


def test_cli_on_the_gpu(dev, tmp_path):
    """gps-sdr-acq without --host (gss_acquire) prints what --host prints, and writes the grid"""
    import subprocess
    data, blk, nch = O.noisy_block(16)
    f, g = tmp_path / "noisy.bin", tmp_path / "grid.bin"
    data.tofile(f)
    args = [G.ACQ_CLI_PATH, "-f", str(f), "-s", str(O.PHYS_FS), "--ncoh=8", "--fmax=5000",
            "--prn=1-3,17,28"]
    gpu = subprocess.run(args + [f"--grid={g}"], capture_output=True, text=True)
    host = subprocess.run(args + ["--host"], capture_output=True, text=True)
    assert gpu.returncode == 0 and host.returncode == 0, gpu.stderr + host.stderr
    assert gpu.stdout == host.stdout and len(gpu.stdout.splitlines()) == 5
    _, want, _ = G.acquire_host(G.Acq(O.PHYS_FS, 16, 1, 8, 500, 10, -1, [1, 2, 3, 17, 28]),
                                data, want_grid=True)
    assert np.array_equal(np.fromfile(g, np.uint64).reshape(want.shape), want)


def test_cli_at_an_odd_window_length(dev, tmp_path):
    """gps-sdr-acq at 1.023 MS/s (L = T = 1023) over the planted peaks: the GPU search prints
    what --host prints, the planted code phases among them, and writes the host's grid"""
    import subprocess
    case = O.SPECIAL_CASES[0]
    fs, coh, M, K, df, prns = case[1]
    assert case[0] == "planted" and prns == tuple(range(1, 18))
    wp, wg, _ = O.answer(case)
    f, g = tmp_path / "planted.bin", tmp_path / "grid.bin"
    O.case_data(case).tofile(f)
    args = [G.ACQ_CLI_PATH, "-f", str(f), "-s", str(fs), f"--ncoh={M}", f"--fmax={K * df}",
            "--prn=1-17"]
    gpu = subprocess.run(args + [f"--grid={g}"], capture_output=True, text=True)
    host = subprocess.run(args + ["--host"], capture_output=True, text=True)
    assert gpu.returncode == 0 and host.returncode == 0, gpu.stderr + host.stderr
    assert gpu.stdout == host.stdout
    rows = [ln.split() for ln in gpu.stdout.splitlines()]
    assert [(int(r[0]), int(r[2]), int(r[3])) for r in rows] == \
        [(int(p["prn"]), int(p["tau"]), int(p["bin"]) * df) for p in wp]
    _, hg, _ = G.acquire_host(acq_of(case[1]), O.case_data(case), want_grid=True)
    assert np.array_equal(np.fromfile(g, np.uint64).reshape(hg.shape), hg)
    assert np.array_equal(hg, wg)
