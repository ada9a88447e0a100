"""Jammers on the GPU (csrc/hip/gss_jam.hip, gss_run with gss_run_opts_t.jam, the CLI's --jam):
every byte against the restatement of tests/jam_oracle.py, and the runs against gss_jam_host over
the plain SC16 run, which the existing parity tests pin to the reference."""
import subprocess

import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import acq_oracle as AO
import jam_oracle as O
from impair_oracle import samples

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
LOC_ARG = "%.6f,%.6f,%g" % LOC


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def jams(js):
    return [O.to_jam(G, j) for j in js]


def on_device(dev, imp, js, iq, s0, fmt, in_off=0, out_off=0, in_place=False):
    """gss_jam_device over iq (host int16[2 n]) placed in_off samples into a device buffer, the
    output out_off bytes into another (or the input's place) between guard bytes; returns the
    bytes"""
    import torch
    n = len(iq) // 2
    nb = G.impair_bytes(n, fmt)
    d_in = torch.zeros(2 * (n + in_off) + 8, dtype=torch.int16, device="cuda")
    d_in[2 * in_off:2 * (in_off + n)] = torch.from_numpy(iq).cuda()
    guard = 64
    d_out = torch.full((nb + out_off + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    p_in = d_in.data_ptr() + 4 * in_off
    p_out = p_in if in_place else d_out.data_ptr() + out_off
    dev.jam_device(imp, jams(js), p_in, s0, n, fmt, p_out)
    torch.cuda.synchronize()
    if in_place:
        got = d_in.cpu().numpy()
        assert (got[:2 * in_off] == 0).all() and (got[2 * (in_off + n):] == 0).all(), "wrote outside"
        return got[2 * in_off:2 * (in_off + n)].view(np.uint8)
    got = d_out.cpu().numpy()
    assert (got[:out_off] == 0xA5).all() and (got[out_off + nb:] == 0xA5).all(), "wrote outside"
    return got[out_off:out_off + nb]


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_jam_device_equals_oracle(dev, fmt):
    """the CPU test's cases without the start 2^64 - 4,100; both NOISE instances"""
    for js, extra in O.cases():
        for sigma, shift in O.NOISE:
            for n in O.SIZES:
                starts = O.STARTS[:-1] + extra if n == 4100 else [1, 2**32 - 5]
                iq = samples(n, seed=n)
                for s0 in starts:
                    got = on_device(dev, G.Impair(sigma, shift, SEED), js, iq, s0, fmt)
                    want = O.jam(SEED, sigma, shift, js, iq, s0, fmt)
                    assert np.array_equal(got, want), (fmt, js, sigma, shift, n, s0)


@pytest.mark.parametrize("sigma", [0, 256 * 300])
def test_levels_and_the_sc16_clamp(dev, sigma):
    iq = samples(4100, seed=9)
    for fmt in (16, 8, 1):
        for amp in (0, 65536, 1 << 23):
            js = [dict(O.CW[0], amp=amp)]
            got = on_device(dev, G.Impair(sigma, 0, SEED), js, iq, 3, fmt)
            assert np.array_equal(got, O.jam(SEED, sigma, 0, js, iq, 3, fmt)), (fmt, amp)
            if fmt == 16 and amp == 1 << 23:
                v = got.view(np.int16)[2:-2]
                assert (v == 32767).sum() > 10 and (v == -32768).sum() > 10


@pytest.mark.parametrize("s0", [0, 1, 2**32 - 5])
def test_jam_device_in_place_sc16(dev, s0):
    for n in (7, 7803):
        iq = samples(n, seed=3)
        for sigma, shift in O.NOISE:
            want = O.jam(SEED, sigma, shift, O.four(), iq, s0, 16)
            for off in (0, 3):
                got = on_device(dev, G.Impair(sigma, shift, SEED), O.four(), iq, s0, 16, in_off=off,
                                in_place=True)
                assert np.array_equal(got, want), (n, off, sigma)


_unaligned = {}


@pytest.mark.parametrize("fmt,in_off,out_off", [
    (16, 1, 4), (16, 3, 12), (16, 1, 8), (16, 0, 2),    # the last two never line up: edges only
    (8, 1, 2), (8, 3, 6), (8, 7, 14), (8, 1, 1),
    (1, 0, 1), (1, 0, 3), (1, 4, 0), (1, 1, 0),
])
def test_jam_device_unaligned_pointers(dev, fmt, in_off, out_off):
    """input and output at every alignment class (tests/test_gpu_impair.py's), four jammers"""
    n = 7804
    iq = samples(n, seed=11)
    for sigma, shift in O.NOISE:
        for s0 in (0, 1):
            key = (fmt, sigma, s0)
            if key not in _unaligned:
                _unaligned[key] = O.jam(SEED, sigma, shift, O.four(), iq, s0, fmt)
            got = on_device(dev, G.Impair(sigma, shift, SEED), O.four(), iq, s0, fmt, in_off, out_off)
            assert np.array_equal(got, _unaligned[key]), (sigma, s0)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_short_sweeps_and_gates_inside_a_group(dev, fmt):
    """P 1, 2, 3 and gate periods 1 and 3 wrap several times inside one thread's 4 / 8 / 16
    samples; P = 16 k + 5 puts a wrap at every position of a group"""
    n = 7804
    iq = samples(n, seed=13)
    sets = [[dict(O.sweeps(P)[i], gate_period=gp, gate_on=gp - (gp > 1), gate_shift=gp - 1)]
            for P in (1, 2, 3) for i in (0, 1) for gp in (1, 3)]
    sets += [[O.sweeps(P)[0], dict(O.sweeps(P)[1], gate_period=P, gate_on=P // 2, gate_shift=3)]
             for P in (5, 21, 37)]
    for js in sets:
        for sigma, shift in O.NOISE:
            for s0 in (0, 2**32 - 1001):
                got = on_device(dev, G.Impair(sigma, shift, SEED), js, iq, s0, fmt)
                assert np.array_equal(got, O.jam(SEED, sigma, shift, js, iq, s0, fmt)), (js, s0)


def test_jam_device_grid_stride(dev):
    """more groups than the capped grid has threads (2,048 x 256 x 4 samples at SC16), four
    jammers, an odd start past 2^33 and a tail"""
    n = 2048 * 256 * 4 + 4099
    iq = samples(n, seed=5)
    s0 = 2**33 + 3
    got = on_device(dev, G.Impair(256 * 300, 1, SEED), O.four(), iq, s0, 16)
    assert np.array_equal(got, O.jam(SEED, 256 * 300, 1, O.four(), iq, s0, 16))


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_no_jammer_is_impair_device(dev, fmt):
    import torch
    n = 7804
    iq = samples(n, seed=17)
    for sigma, shift in O.NOISE:
        imp = G.Impair(sigma, shift, SEED)
        d_in = torch.from_numpy(iq).cuda()
        d_out = torch.zeros(G.impair_bytes(n, fmt), dtype=torch.uint8, device="cuda")
        dev.impair_device(imp, d_in.data_ptr(), 2**32 - 77, n, fmt, d_out.data_ptr())
        torch.cuda.synchronize()
        want = d_out.cpu().numpy()
        assert np.array_equal(on_device(dev, imp, [], iq, 2**32 - 77, fmt), want)
        assert np.array_equal(G.jam_host(imp, [], iq, 2**32 - 77, fmt), want)


def test_jam_device_argument_errors(dev):
    """refused before any launch: the output keeps its guard pattern"""
    import torch
    d_in = torch.zeros(64, dtype=torch.int16, device="cuda")
    d_out = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    pi, po = d_in.data_ptr(), d_out.data_ptr()
    ok, imp = G.Jam(step0=1, amp=65536), G.Impair(0, 0, 0)
    bad = [G.Jam(sweep=0), G.Jam(amp=(1 << 23) + 1), G.Jam(gate_period=4, gate_on=5),
           G.Jam(gate_period=4, gate_on=1, gate_shift=4), G.Jam(gate_shift=1), G.Jam(pad=1)]
    calls = [(imp, [ok, b], 8, 16, po) for b in bad]
    calls += [(imp, [ok] * 5, 8, 16, po), (G.Impair(1, 9, 0), [ok], 8, 16, po),
              (G.Impair(0x1000000, 0, 0), [ok], 8, 16, po), (imp, [ok], 8, 4, po),
              (imp, [ok], 6, 1, po), (imp, [ok], 8, 8, pi), (imp, [ok], 8, 1, pi),
              (imp, [ok], 8, 16, 0)]
    for p, js, n, fmt, out in calls:
        with pytest.raises(G.GssError) as e:
            dev.jam_device(p, js, pi, 0, n, fmt, out)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all() and (d_in.cpu().numpy() == 0).all()


# ---- runs ----------------------------------------------------------------------------------------
FS = 1000000
IMP = {16: (256 * 300, 1), 8: (256 * 300, 3), 1: (256 * 300, 0)}      # (sigma_q8, shift)


def run_jams():
    """a pulsed tone 10 dB up and a sweep at the satellites' level, as tests/helpers/jam_fake.cpp"""
    a = G.jam_make(FS, 10.0, 137e3, 0.0, 0.0, 10e-6, 0.3)
    a.gate_shift = 7
    b = G.jam_make(FS, 0.0, -400e3, 400e3, 137e-6)
    b.phase0 = 0x8000000000000001
    return [a, b]


def run_bytes(dev, fmt, impair=None, jam=None, **kw):
    s = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(FS), data_format=fmt)
    parts, seen = [], []

    def sink(buf, first, nb):
        parts.append(bytes(buf))
        seen.append((first, nb))

    dev.run(s, sink, impair=impair, jam=jam, **kw)
    npb = s.n_per_blk
    s.close()
    for (a, na), (b, _) in zip(seen, seen[1:]):
        assert a + na == b
    return np.frombuffer(b"".join(parts), np.uint8), npb, seen


_run = {}


@pytest.fixture(scope="module")
def expected(dev):
    """fmt -> (gss_jam_host over the plain -b 16 run, gss_impair_host over it, n_per_blk):
    the plain run once, each format's bytes once"""
    def get(fmt):
        if "iq" not in _run:
            raw, npb, _ = run_bytes(dev, 16, batch=128)
            _run["iq"] = (raw.view(np.int16), npb)
            assert len(raw) == 4 * 9 * npb
        iq, npb = _run["iq"]
        if fmt not in _run:
            imp = G.Impair(*IMP[fmt], 7)
            _run[fmt] = (G.jam_host(imp, run_jams(), iq, 0, fmt), G.impair_host(imp, iq, 0, fmt))
        return _run[fmt] + (npb,)
    return get


MODES = {
    "batch2": ({}, dict(batch=2)),
    "batch128": ({}, dict(batch=128)),
    "range": ({}, dict(batch=3, first_block=3, n_blocks=4)),
    "gpu_exact3_late": ({"GSS_RUN_PROOF": "gpu", "GSS_RUN_FORCE_EXACT": "3",
                         "GSS_RUN_LATE_VERDICTS": "1"}, dict(batch=4)),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_run_with_noise_and_jammers(dev, expected, monkeypatch, fmt, mode):
    want, _, npb = expected(fmt)                    # (the plain run before the mode's environment)
    env, kw = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, _, seen = run_bytes(dev, fmt, impair=G.Impair(*IMP[fmt], 7), jam=run_jams(), threads=4, **kw)
    if mode == "range":
        bb = G.block_bytes(npb, fmt)
        assert seen[0][0] == 3 and sum(nb for _, nb in seen) == 4
        assert np.array_equal(got, want[3 * bb:7 * bb])
    else:
        assert sum(nb for _, nb in seen) == 9
        assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_run_without_jammers_is_todays(dev, expected, fmt):
    """jam=None and jam=[]: the impairment's bytes; jammers without an impairment: refused"""
    _, want, _ = expected(fmt)
    for jam in (None, []):
        got, _, _ = run_bytes(dev, fmt, impair=G.Impair(*IMP[fmt], 7), jam=jam, batch=4)
        assert np.array_equal(got, want)
    with pytest.raises(G.GssError) as e:
        run_bytes(dev, fmt, impair=None, jam=run_jams(), batch=4)
    assert e.value.code == -1


def test_jammers_alone_through_the_run(dev, expected):
    """sigma 0: the NOISE = false instance inside gss_run"""
    expected(8)
    iq, _ = _run["iq"]
    imp = G.Impair(0, 2, 0)
    got, _, _ = run_bytes(dev, 8, impair=imp, jam=run_jams(), batch=5)
    assert np.array_equal(got, G.jam_host(imp, run_jams(), iq, 0, 8))


def test_cli_jam(dev, expected, tmp_path):
    """gps-sdr-sim --jam=... writes gss_jam_host over the plain run, with the jammers the parser
    resolves, and one stderr line per jammer"""
    expected(8)
    iq, _ = _run["iq"]
    opts = ["--cn0=45", "--seed=7", "--jam=cw,10,137e3,pulse,10e-6,0.3",
            "--jam=sweep,0,-400e3,400e3,137e-6"]
    out = tmp_path / "jammed.bin"
    p = subprocess.run([G.CLI_PATH, "-e", NAV, "-l", LOC_ARG, "-d", "1", "-s", str(FS), "-b", "8",
                        "-o", str(out)] + opts, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr.count("\nJammer ") == 2 and "Noise: " in p.stderr
    scn, _ = G.Scenario.from_cli(["-e", NAV, "-l", LOC_ARG, "-d", "1", "-s", str(FS), "-b", "8"]
                                 + opts)
    imp, js = scn.impair, scn.jam
    scn.close()
    assert len(js) == 2 and js[0].gate_period == 10 and js[1].sweep == 137
    assert np.array_equal(np.fromfile(out, np.uint8), G.jam_host(imp, js, iq, 0, 8))


# ---- end to end ------------------------------------------------------------------------------------
PHYS_SIGMA = int(np.floor(256 * 250 * np.sqrt(AO.PHYS_FS / (2 * 10 ** (AO.PHYS_CN0 / 10))) + 0.5))


@pytest.mark.parametrize("fmt", [16, 8])
@pytest.mark.parametrize("js_db,shifts,found", [(0.0, {16: 0, 8: 2}, True),
                                                (30.0, {16: 0, 8: 5}, False)])
def test_end_to_end(dev, js_db, shifts, found, fmt):
    """gss_run with noise at 50 dB-Hz and a tone at 0 Hz, the search over the run's first block
    on the device: the host's peaks; at J/S 0 dB the eleven satellites found where the rows say,
    at 30 dB no PRN at the threshold"""
    fs = AO.PHYS_FS
    imp = G.Impair(PHYS_SIGMA, shifts[fmt], 7)
    s = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(fs), data_format=fmt)
    bb = G.block_bytes(s.n_per_blk, fmt)
    first = []

    def sink(buf, b0, nb):
        if b0 == 0:
            first.append(np.frombuffer(bytes(buf[:bb]), np.uint8))

    dev.run(s, sink, batch=4, impair=imp, jam=[G.jam_make(float(fs), js_db, 0.0)])
    s.close()
    rows = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(fs))
    blk, nch = rows.next(1)
    rows.close()
    acq = AO.PHYS_ACQ(fmt)
    peaks, _, sh = dev.acquire_from_host(acq, first[0])
    hp, _, hsh = G.acquire_host(acq, first[0])
    assert sh == hsh and np.array_equal(peaks, hp)
    if found:
        AO.check_physical(peaks, blk, nch, level=False, found=True)
    else:
        ratios = [G.acq_ratio(p) for p in peaks]
        print("largest ratio %.2f against %.2f" % (max(ratios), AO.phys_threshold()))
        assert len(ratios) == 32 and max(ratios) < AO.phys_threshold()


def test_run_node_refuses_jammers():
    from gpssim_amd.node import run_node
    with pytest.raises(ValueError, match="jam"):
        run_node(["-e", NAV, "-l", LOC_ARG, "-d", "1", "--jam=cw,0,0"], 0, 1, 0)
