"""The front-end filter on the GPU (csrc/hip/gss_fir.hip, gss_run with gss_run_opts_t.fir, the
CLI's --bandwidth): every byte against the restatement of tests/fir_oracle.py in both forms of
the kernel, and the runs against gss_fir_host over gss_jam_host over gss_echo_host over the plain
SC16 run, which the existing parity tests pin to the reference."""
import subprocess

import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import acq_oracle as AO
import fir_oracle as O

pytestmark = pytest.mark.gpu

LOC_ARG = "%.6f,%.6f,%g" % LOC
PATHS = ["staged", "plain"]
NS = (1, 2, 3, 7, 33, 62, 63, 64, 1023, 1025, 4099)
TS = (1, 2, 3, 31, 63, 64)
GRID_MAX = 2048
TILE = {16: 1024, 8: 2048, 1: 4096}          # samples per workgroup and trip


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    if request.param == "plain":
        monkeypatch.setenv("GSS_FIR_PATH", "plain")
    else:
        monkeypatch.delenv("GSS_FIR_PATH", raising=False)
    return request.param


def sizes(fmt):
    return NS if fmt != 1 else tuple(sorted({(n + 3) // 4 * 4 for n in NS}))


def samples(rng, n):
    return rng.integers(-32768, 32768, 2 * n).astype(np.int16)


def on_device(dev, taps, x, halo, fmt, off_in=0, off_out=0):
    """gss_fir_device over x (host int16[2 n]) placed off_in bytes into a device buffer, its
    output off_out bytes into another between guard bytes; returns the output's bytes"""
    import torch
    f = taps if isinstance(taps, G.Fir) else G.Fir(taps)
    n = len(x) // 2
    nb = G.impair_bytes(n, fmt)
    guard = 64
    d_in = torch.full((guard + off_in + 4 * n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out = torch.full((guard + off_out + nb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    li, lo = guard + off_in, guard + off_out
    d_in[li:li + 4 * n] = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).cuda()
    d_halo = None
    if halo is not None and len(halo):
        d_halo = torch.from_numpy(np.ascontiguousarray(halo).view(np.uint8)).cuda()
    dev.fir_device(f, d_in.data_ptr() + li, d_halo.data_ptr() if d_halo is not None else 0, n, fmt,
                   d_out.data_ptr() + lo)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[:lo] == 0xA5).all() and (got[lo + nb:] == 0xA5).all(), "wrote outside"
    assert (d_in.cpu().numpy()[:li] == 0xA5).all()
    return got[lo:lo + nb].copy()


_cases = {}


def cases(fmt, T):
    """(taps, x, halo, want without halo, want with halo) for every n; the oracle once for both
    forms of the kernel"""
    if (fmt, T) not in _cases:
        rng = np.random.default_rng(1000 * fmt + T)
        out = []
        for n in sizes(fmt):
            taps, x, halo = O.random_taps(rng, T), samples(rng, n), samples(rng, T - 1)
            out.append((taps, x, halo, O.fir(taps, x, None, fmt), O.fir(taps, x, halo, fmt)))
        _cases[(fmt, T)] = out
    return _cases[(fmt, T)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_fir_device_equals_oracle(dev, path, fmt, T):
    """the CPU list of n and T (n shorter than T - 1 among them), a null halo and a given one"""
    for taps, x, halo, want0, want1 in cases(fmt, T):
        assert np.array_equal(on_device(dev, taps, x, None, fmt), want0), len(x) // 2
        assert np.array_equal(on_device(dev, taps, x, halo, fmt), want1), len(x) // 2


@pytest.mark.parametrize("off", [0, 2, 4, 6, 8, 10, 12, 14])
@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_fir_device_unaligned(dev, path, fmt, off):
    """in and out at every 2-byte offset class of a 16-byte line (SC08 and SC01 outputs at the
    odd bytes too): the classes that line up take heads of 0..3 samples, the others go by the
    edges alone"""
    taps, x, halo, _, want = cases(fmt, 63)[-1]              # n = 4099 (4100)
    assert np.array_equal(on_device(dev, taps, x, halo, fmt, off, 0), want)
    assert np.array_equal(on_device(dev, taps, x, halo, fmt, 0, off), want)
    assert np.array_equal(on_device(dev, taps, x, halo, fmt, off, off), want)
    assert np.array_equal(on_device(dev, taps, x, halo, fmt, off, (off + 4) % 16), want)
    if fmt != 16:
        assert np.array_equal(on_device(dev, taps, x, halo, fmt, off, off // 2 + 1), want)
    taps, x, halo, _, want = cases(fmt, 64)[3]               # n = 7 (8)
    assert np.array_equal(on_device(dev, taps, x, halo, fmt, off, off), want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_fir_device_at_the_ends_of_int32(dev, path, fmt):
    n = 68
    low = np.full(2 * n, -32768, np.int16)
    for T in TS:
        halo = np.full(2 * (T - 1), -32768, np.int16)
        for sign in (1, -1):
            taps = O.extreme_taps(T, sign)
            assert np.array_equal(on_device(dev, taps, low, halo, fmt), O.fir(taps, low, halo, fmt))
        taps = O.extreme_taps(T, 0)
        for level in (32767, -32767):
            x = O.sign_matched(taps, n, 65, level)
            assert np.array_equal(on_device(dev, taps, x, None, fmt), O.fir(taps, x, None, fmt))


_stride = {}


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_fir_device_grid_stride(dev, path, fmt):
    """one call that passes the grid stride once: cap x tile + 4,099 samples (SC01: + 4,100),
    T = 64, random data, against the oracle over the whole range, computed once for both forms"""
    if fmt not in _stride:
        rng = np.random.default_rng(40 + fmt)
        n = GRID_MAX * TILE[fmt] + (4099 if fmt != 1 else 4100)
        taps, x, halo = O.random_taps(rng, 64), samples(rng, n), samples(rng, 63)
        want = O.fir(taps, x, halo, fmt)
        _stride[fmt] = (taps, x, halo, want)
    taps, x, halo, want = _stride[fmt]
    assert np.array_equal(on_device(dev, taps, x, halo, fmt), want)


def test_fir_device_argument_errors(dev, path, monkeypatch):
    """refused before any launch: the output keeps its pattern"""
    import torch
    d_in = torch.zeros(256, dtype=torch.int16, device="cuda")
    d_out = torch.full((512,), 0x5A, dtype=torch.uint8, device="cuda")
    ok = G.Fir([8192, 8192])
    good = dict(f=ok, x=d_in.data_ptr(), halo=0, n=64, fmt=16, out=d_out.data_ptr())
    bad = [dict(f=G.Fir([1], n_taps=0)), dict(f=G.Fir([1], n_taps=65)), dict(f=G.Fir([1, 2], pad=1)),
           dict(f=G.Fir([32767, 32767, 2])), dict(fmt=4), dict(fmt=1, n=62), dict(x=0), dict(out=0),
           dict(x=d_in.data_ptr() + 1), dict(out=d_out.data_ptr() + 1), dict(halo=d_in.data_ptr() + 1),
           dict(out=d_in.data_ptr()), dict(out=d_in.data_ptr() + 4 * 63),
           dict(x=d_in.data_ptr() + 8, out=d_in.data_ptr(), fmt=8)]
    for b in bad:
        a = dict(good, **b)
        with pytest.raises(G.GssError) as e:
            dev.fir_device(a["f"], a["x"], a["halo"], a["n"], a["fmt"], a["out"])
        assert e.value.code == -1, b
    monkeypatch.setenv("GSS_FIR_PATH", "fast")
    with pytest.raises(G.GssError) as e:
        dev.fir_device(ok, good["x"], 0, 64, 16, good["out"])
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()


# ---- runs ----------------------------------------------------------------------------------------
FS = 1000000
DURATION = 0.5
IMP = {16: (256 * 300, 1), 8: (256 * 300, 3), 1: (256 * 300, 0)}      # (sigma_q8, shift)


def run_jam():
    return [G.jam_make(FS, 10.0, 437e3)]


def run_echoes():
    """an echo of every satellite 150 m late, 6 dB down, fading at 2.5 Hz"""
    return [G.echo_make(FS, 0, 150.0, 6.0, 30.0, 2.5)]


def run_fir():
    return G.fir_make(FS, 700e3, 63)


def run_bytes(dev, fmt, impair=None, jam=None, echo=None, fir=None, **kw):
    s = G.Scenario(NAV, llh=LOC, duration=DURATION, samp_freq=float(FS), data_format=fmt)
    parts, seen = [], []

    def sink(buf, first, nb):
        parts.append(bytes(buf))
        seen.append((first, nb))

    dev.run(s, sink, impair=impair, jam=jam, echo=echo, fir=fir, **kw)
    npb = s.n_per_blk
    s.close()
    for (a, na), (b, _) in zip(seen, seen[1:]):
        assert a + na == b
    return np.frombuffer(b"".join(parts), np.uint8), npb, seen


_run = {}


@pytest.fixture(scope="module")
def expected(dev):
    """fmt -> (gss_fir_host over gss_jam_host (SC16) over gss_echo_host over the plain -b 16 run
    as one stream, gss_jam_host over gss_echo_host in the format without the filter, n_per_blk):
    the plain run and the echoes' samples once, each format's bytes once"""
    def get(fmt):
        if "iq" not in _run:
            raw, npb, _ = run_bytes(dev, 16, batch=128)
            nblk = len(raw) // (4 * npb)
            rows = G.Scenario(NAV, llh=LOC, duration=DURATION, samp_freq=float(FS))
            blk, nch = rows.all_blocks()
            nav = rows.nav_table()
            rows.close()
            assert len(nch) == nblk
            iq = raw.view(np.int16)
            mid = G.echo_host(run_echoes(), blk, nch, G.ca_table(), nav, npb, 0, iq)
            _run["iq"] = (iq, mid, npb)
        iq, mid, npb = _run["iq"]
        if fmt not in _run:
            imp = G.Impair(*IMP[fmt], 7)
            sc16 = G.jam_host(imp, run_jam(), mid, 0, 16).view(np.int16)
            want = G.fir_host(run_fir(), sc16, None, fmt)
            plain = G.jam_host(imp, run_jam(), mid, 0, fmt)
            assert not np.array_equal(want, plain)
            _run[fmt] = (want, plain)
        return _run[fmt] + (npb,)
    return get


MODES = {
    "batch2": ({}, dict(batch=2)),
    "batch128": ({}, dict(batch=128)),
    "range": ({}, dict(batch=3, first_block=1, n_blocks=2)),
    "gpu_exact3_late": ({"GSS_RUN_PROOF": "gpu", "GSS_RUN_FORCE_EXACT": "3",
                         "GSS_RUN_LATE_VERDICTS": "1"}, dict(batch=4)),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_run_with_noise_a_jammer_an_echo_and_the_filter(dev, expected, monkeypatch, fmt, mode):
    want, _, npb = expected(fmt)                    # (the plain run before the mode's environment)
    env, kw = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, _, seen = run_bytes(dev, fmt, impair=G.Impair(*IMP[fmt], 7), jam=run_jam(),
                             echo=run_echoes(), fir=run_fir(), threads=4, **kw)
    nblk = len(want) // G.block_bytes(npb, fmt)
    if mode == "range":
        bb = G.block_bytes(npb, fmt)
        assert seen[0][0] == 1 and sum(nb for _, nb in seen) == 2
        assert np.array_equal(got, want[bb:3 * bb])
    else:
        assert sum(nb for _, nb in seen) == nblk
        assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_run_without_the_filter_is_the_parents(dev, expected, fmt):
    """fir=None: the bytes of the run with the other three options; a filter without an
    impairment: refused"""
    _, want, _ = expected(fmt)
    got, _, _ = run_bytes(dev, fmt, impair=G.Impair(*IMP[fmt], 7), jam=run_jam(), echo=run_echoes(),
                          fir=None, batch=4)
    assert np.array_equal(got, want)
    with pytest.raises(G.GssError) as e:
        run_bytes(dev, fmt, impair=None, fir=run_fir(), batch=4)
    assert e.value.code == -1


def test_cli_bandwidth(dev, expected, tmp_path):
    """gps-sdr-sim --bandwidth=... writes the host composition over the plain run, with the
    options the parser resolves, and one stderr line for the filter"""
    _, _, npb = expected(8)
    iq, _, _ = _run["iq"]
    opts = ["--cn0=45", "--seed=7", "--jam=cw,10,437e3", "--multipath=all,150,6,30,2.5",
            "--bandwidth=700000"]
    args = ["-e", NAV, "-l", LOC_ARG, "-d", str(DURATION), "-s", str(FS), "-b", "8"]
    out = tmp_path / "filtered.bin"
    p = subprocess.run([G.CLI_PATH] + args + ["-o", str(out)] + opts, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Filter: taps = 63, delay = 31 samples, noise gain = 0.68928" in p.stderr
    scn, _ = G.Scenario.from_cli(args + opts)
    imp, js, es, f = scn.impair, scn.jam, scn.echo, scn.fir
    blk, nch = scn.all_blocks()
    nav = scn.nav_table()
    scn.close()
    mid = G.echo_host(es, blk, nch, G.ca_table(), nav, npb, 0, iq)
    sc16 = G.jam_host(imp, js, mid, 0, 16).view(np.int16)
    assert np.array_equal(np.fromfile(out, np.uint8), G.fir_host(f, sc16, None, 8))


PHYS_SIGMA = int(np.floor(256 * 250 * np.sqrt(AO.PHYS_FS / (2 * 10 ** (AO.PHYS_CN0 / 10))) + 0.5))


def test_end_to_end_behind_the_filter(dev):
    """gss_run with noise at 50 dB-Hz, a tone 30 dB up at 450 kHz and the 700 kHz filter, the
    search over the run's first block on the device: the host's peaks, the eleven satellites
    within one bin and one sample of tau + 31 and over the threshold, the absent PRNs under it"""
    fs, fmt = AO.PHYS_FS, 8
    imp = G.Impair(PHYS_SIGMA, 2, 7)
    s = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(fs), data_format=fmt)
    bb = G.block_bytes(s.n_per_blk, fmt)
    first = []

    def sink(buf, b0, nb):
        if b0 == 0:
            first.append(np.frombuffer(bytes(buf[:bb]), np.uint8))

    dev.run(s, sink, batch=4, impair=imp, jam=[G.jam_make(float(fs), 30.0, 450e3)],
            fir=G.fir_make(float(fs), 700e3, 63))
    s.close()
    rows = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(fs))
    blk, nch = rows.next(1)
    rows.close()
    acq = AO.PHYS_ACQ(fmt)
    peaks, _, sh = dev.acquire_from_host(acq, first[0])
    hp, _, hsh = G.acquire_host(acq, first[0])
    assert sh == hsh and np.array_equal(peaks, hp)
    p = peaks.copy()
    p["tau"] = (p["tau"] - O.group_delay(63)) % 1000
    AO.check_physical(p, blk, nch, level=False, found=True)
