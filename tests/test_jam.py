"""Jammers at a chosen J/S (include/gpssim_amd.h, gss_jam_t), the parts that need no GPU: the host
statement gss_jam_host against the restatement of tests/jam_oracle.py byte for byte, gss_jam_make
against its formulas, the physics of a tone, a sweep and a pulse, the command-line option,
gss_run with jammers on the CPU fakes of tests/helpers (jam_fake.cpp), and what a tone does to
the acquisition search."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import NAV, REPO
from fake_build import programs

import gpssim_amd as G
import acq_oracle as AO
import jam_oracle as O
from impair_oracle import samples

SEED = 0x9E3779B97F4A7C15


def jams(js):
    return [O.to_jam(G, j) for j in js]


def host(sigma, shift, js, iq, s0, fmt, seed=SEED):
    return G.jam_host(G.Impair(sigma, shift, seed), jams(js), iq, s0, fmt)


cases = O.cases


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_jam_host_equals_oracle(fmt):
    """every case at n = 4,100 from every start; the short sizes from the starts that put an
    odd index and 2^32 inside them.  2^64 - 4,100 takes the short sizes only: a range that ends
    at 2^64 is an argument error of gss_impair_check (asserted)."""
    for js, extra in cases():
        for sigma, shift in O.NOISE:
            for n in O.SIZES:
                starts = O.STARTS + extra if n == 4100 else [1, 2**32 - 5, 2**64 - 4100]
                iq = samples(n, seed=n)
                for s0 in starts:
                    if s0 + n >= 2**64:
                        with pytest.raises(G.GssError):
                            host(sigma, shift, js, iq, s0, fmt)
                        continue
                    got = host(sigma, shift, js, iq, s0, fmt)
                    want = O.jam(SEED, sigma, shift, js, iq, s0, fmt)
                    assert got.shape == want.shape == (G.impair_bytes(n, fmt),)
                    assert np.array_equal(got, want), (fmt, js, sigma, shift, n, s0)


@pytest.mark.parametrize("sigma", [0, 256 * 300])
def test_levels_and_the_sc16_clamp(sigma):
    """amp 0, 65536 and 2^23 at shift 0: the largest writes 32,000 beside the input, so the SC16
    clamp fires on both rails"""
    n = 4100
    iq = samples(n, seed=9)
    for fmt in (16, 8, 1):
        for amp in (0, 65536, 1 << 23):
            js = [dict(O.CW[0], amp=amp)]
            got = host(sigma, 0, js, iq, 3, fmt)
            assert np.array_equal(got, O.jam(SEED, sigma, 0, js, iq, 3, fmt)), (fmt, amp)
            if fmt == 16 and amp == 1 << 23:
                v = got.view(np.int16)[2:-2]
                assert (v == 32767).sum() > 10 and (v == -32768).sum() > 10
    assert np.array_equal(host(sigma, 0, [dict(O.CW[0], amp=0)], iq, 3, 16),
                          G.impair_host(G.Impair(sigma, 0, SEED), iq, 3, 16))


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_no_jammer_is_the_impairment_and_ranges_compose(fmt):
    iq = samples(96)
    a = 2**32 - 40
    for sigma, shift in O.NOISE:
        imp = G.Impair(sigma, shift, 99)
        assert np.array_equal(G.jam_host(imp, [], iq, a, fmt), G.impair_host(imp, iq, a, fmt))
        whole = G.jam_host(imp, jams(O.four(7)), iq, a, fmt)
        for cut in ([33, 64] if fmt != 1 else [32, 64]):
            parts = np.concatenate([G.jam_host(imp, jams(O.four(7)), iq[:2 * cut], a, fmt),
                                    G.jam_host(imp, jams(O.four(7)), iq[2 * cut:], a + cut, fmt)])
            assert np.array_equal(parts, whole), cut


def test_jam_host_in_place_sc16():
    iq = samples(1001)
    imp = G.Impair(256 * 300, 1, 5)
    js = jams(O.four())
    want = G.jam_host(imp, js, iq, 77, 16)
    buf = iq.copy()
    p = C.c_void_p(buf.ctypes.data)
    arr = (G.Jam * 4)(*js)
    assert G.lib().gss_jam_host(C.byref(imp), arr, 4, p, 77, 1001, 16, p) == 0
    assert np.array_equal(buf.view(np.uint8), want)


BAD_JAMS = [dict(sweep=0), dict(amp=(1 << 23) + 1), dict(gate_period=4, gate_on=5),
            dict(gate_period=4, gate_on=1, gate_shift=4), dict(gate_shift=1), dict(pad=1)]


def test_jam_host_argument_errors():
    iq = samples(8)
    out = np.full(64, 0xA5, np.uint8)
    pi, po = C.c_void_p(iq.ctypes.data), C.c_void_p(out.ctypes.data)
    f = G.lib().gss_jam_host
    imp = C.byref(G.Impair(0, 0, 0))
    good = (G.Jam * 5)(*[G.Jam(step0=1, amp=1 << 23, gate_period=4, gate_on=4, gate_shift=3)] * 5)
    assert f(imp, good, 4, pi, 0, 8, 16, po) == 0
    out[:] = 0xA5
    for bad in BAD_JAMS:
        arr = (G.Jam * 2)(G.Jam(step0=1), G.Jam(**bad))
        assert f(imp, arr, 2, pi, 0, 8, 16, po) == -1, bad
        assert f(imp, arr, 1, pi, 0, 8, 16, po) == 0, bad      # the bad one is not among them
        out[:] = 0xA5
    assert f(imp, good, 5, pi, 0, 8, 16, po) == -1
    assert f(imp, good, -1, pi, 0, 8, 16, po) == -1
    assert f(imp, None, 1, pi, 0, 8, 16, po) == -1
    assert f(None, good, 1, pi, 0, 8, 16, po) == -1                    # p is required
    assert f(C.byref(G.Impair(1, 9, 0)), good, 1, pi, 0, 8, 16, po) == -1
    assert f(imp, good, 1, pi, 0, 6, 1, po) == -1                      # SC01: n % 4
    assert f(imp, good, 1, pi, 0, 8, 8, pi) == -1                      # in place: SC16 only
    assert f(imp, good, 1, None, 0, 8, 16, po) == -1
    assert f(imp, good, 1, pi, 2**64 - 4, 8, 16, po) == -1
    assert (out == 0xA5).all()
    with pytest.raises(G.GssError) as e:
        G.jam_host(G.Impair(0, 0, 0), [G.Jam()] * 5, iq, 0, 16)
    assert e.value.code == -1


MAKE = [
    (1e6, 0.0, 137e3, 0.0, 0.0, 0.0, 0.0), (1e6, 30.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    (2.6e6, -12.5, -1.2999e6, 0.0, 0.0, 0.0, 0.0), (1e6, 42.1, -137e3, 0.0, 0.0, 1e-3, 0.1),
    (1e6, 0.0, -400e3, 400e3, 137e-6, 0.0, 0.0), (1e6, 3.0, 400e3, -400e3, 1e-3, 0.0, 0.0),
    (2.6e6, 10.0, -1e6, 1e6, 1.0, 2e-3, 0.25), (1e6, 0.0, 1.0, 3.0, 4294.967295, 0.0, 0.0),
    (1e6, 0.0, 100.0, 100.0, 1e-6, 1e-6, 1.0), (1e6, -200.0, 0.0, 0.0, 0.0, 1e-5, 0.0),
    (1000010.0, 6.0, -499e3, 499e3, 0.1, 0.05, 0.5),
]


@pytest.mark.parametrize("args", MAKE)
def test_jam_make(args):
    got, want = G.jam_make(*args), O.make(*args)
    assert {k: getattr(got, k) for k in want} == want and got.pad == 0


@pytest.mark.parametrize("args", [
    (1e6, 42.2, 0, 0, 0, 0, 0), (1e6, 0, 500e3, 0, 0, 0, 0), (1e6, 0, -500e3, 0, 0, 0, 0),
    (1e6, 0, 0, 500e3, 1e-3, 0, 0), (1e6, 0, 0, 1, 1e-9, 0, 0), (1e6, 0, 0, 1, 5000.0, 0, 0),
    (1e6, 0, 0, 1, -1.0, 0, 0), (1e6, 0, 0, 0, 0, 1e-3, 1.5), (1e6, 0, 0, 0, 0, 1e-3, -0.1),
    (1e6, 0, 0, 0, 0, 1e-9, 0.5), (1e6, 0, 0, 0, 0, 5000.0, 0.5), (1e6, 0, 0, 0, 0, -1.0, 0.5),
    (0.0, 0, 0, 0, 0, 0, 0), (-1e6, 0, 0, 0, 0, 0, 0), (1e6, float("nan"), 0, 0, 0, 0, 0),
    (1e6, 0, float("inf"), 0, 0, 0, 0), (float("nan"), 0, 0, 0, 0, 0, 0),
])
def test_jam_make_rejections(args):
    with pytest.raises(G.GssError) as e:
        G.jam_make(*args)
    assert e.value.code == -1


# ---- physics on zero input, SC16, shift 0 ------------------------------------------------------
def jammer_alone(j, n, s0=0):
    z = np.zeros(2 * n, np.int16)
    v = G.jam_host(G.Impair(0, 0, 0), [j], z, s0, 16).view(np.int16).astype(np.float64)
    return v[0::2] + 1j * v[1::2]


def test_tone_power_and_line():
    n, fs = 100000, 1e6
    x = jammer_alone(G.jam_make(fs, 0.0, 137e3), n)
    db = 10 * np.log10((np.abs(x) ** 2).mean() / 250.0 ** 2)
    e = np.abs(np.fft.fft(x)) ** 2
    peak = int(e.argmax())
    print("tone: power %+.4f dB, peak bin %d, share %.6f" % (db, peak, e[peak] / e.sum()))
    assert abs(db) <= 0.01
    assert peak == 13700 and e[peak] / e.sum() > 0.9999


def test_sweep_fills_its_band():
    n, fs = 100000, 1e6
    j = G.jam_make(fs, 0.0, -400e3, 400e3, 1e-3)
    assert j.sweep == 1000
    x = jammer_alone(j, n)
    e = np.abs(np.fft.fft(x)) ** 2
    f = np.fft.fftfreq(n, 1 / fs)
    share = e[np.abs(f) <= 400e3].sum() / e.sum()
    print("sweep: share inside the band %.4f" % share)
    assert share >= 0.98


@pytest.mark.parametrize("period,on,shift", [(10, 3, 0), (10, 3, 9), (1000, 1, 999), (7, 7, 3),
                                             (7, 0, 0), (1, 1, 0), (1, 0, 0)])
def test_gate_counts(period, on, shift):
    n, s0 = 100003, 2**32 - 50001
    for amp in (65536, 1 << 23):
        j = G.Jam(step0=O.step_of(137e3, 1e6), amp=amp, gate_period=period, gate_on=on,
                  gate_shift=shift)
        x = jammer_alone(j, n, s0)
        idx = np.arange(n, dtype=np.uint64) + np.uint64(s0)
        want = ((idx % np.uint64(period)) + np.uint64(shift)) % np.uint64(period) < np.uint64(on)
        assert np.array_equal(x != 0, want)              # amp >= 65536: an on-sample is never (0, 0)
        assert int((x != 0).sum()) == int(want.sum())


# ---- the command line --------------------------------------------------------------------------
def parse(*args):
    cli = G._Cli()
    argv = [b"gps-sdr-sim", b"-e", NAV.encode()] + [a.encode() for a in args]
    arr = (C.c_char_p * len(argv))(*argv)
    return G.lib().gss_cli_parse(len(argv), arr, C.byref(cli)), cli


def as_dict(j):
    return {k: getattr(j, k) for k in O.J()}


def test_cli_jam_forms():
    fs = 1e6
    rc, cli = parse("-s", "1000000", "-b", "16")
    assert rc == 0 and cli.n_jam == 0 and cli.has_impair == 0
    rc, cli = parse("--cn0=45", "-s", "1000000", "-b", "8")          # today's impair, no jammer
    assert rc == 0 and cli.n_jam == 0 and cli.has_impair == 1 and cli.impair.shift == 2
    forms = [("cw,0,137000", (0.0, 137e3)),
             ("cw,30,-1.5e3,pulse,1e-3,0.1", (30.0, -1.5e3, 0.0, 0.0, 1e-3, 0.1)),
             ("sweep,0,-400e3,400e3,137e-6", (0.0, -400e3, 400e3, 137e-6)),
             ("sweep,12.5,400e3,-400e3,1e-3,pulse,2e-3,0.5", (12.5, 400e3, -400e3, 1e-3, 2e-3, 0.5))]
    for text, args in forms:                 # the option before -s: resolved at the run's rate
        rc, cli = parse("--jam=" + text, "-s", "1000000", "-b", "8")
        assert rc == 0 and cli.n_jam == 1 and cli.has_impair == 1, text
        assert as_dict(cli.jam[0]) == O.make(fs, *args), text
        assert (cli.impair.sigma_q8, cli.impair.seed) == (0, 0)
    rc, cli = parse("-s", "1000000", *["--jam=" + t for t, _ in forms])
    assert rc == 0 and cli.n_jam == 4
    for i, (_, args) in enumerate(forms):
        assert as_dict(cli.jam[i]) == O.make(fs, *args)
    rc, cli = parse("-s", "1000000", *["--jam=" + t for t, _ in forms], "--jam=cw,0,0")
    assert rc == 1


def auto_shift(sigma_q8, amps, room):
    peak = 4.0 * (sigma_q8 / 256.0) + 2047.0 + sum(a * 250.0 / 65536.0 for a in amps)
    return min(s for s in range(9) if peak <= room * 2**s or s == 8)


def test_cli_auto_shift_with_a_jammer():
    for b, room in (("16", 32767.0), ("8", 2047.0)):
        for js in ("0", "20", "30", "42.1"):
            rc, cli = parse("-s", "1000000", "-b", b, "--jam=cw," + js + ",0")
            assert rc == 0 and cli.impair.sigma_q8 == 0
            assert cli.impair.shift == auto_shift(0, [cli.jam[0].amp], room), (b, js)
            rc, cli = parse("-s", "1000000", "-b", b, "--cn0=45", "--jam=cw," + js + ",0",
                            "--jam=cw,10,1000")
            assert rc == 0 and cli.n_jam == 2
            assert cli.impair.shift == auto_shift(cli.impair.sigma_q8,
                                                  [cli.jam[0].amp, cli.jam[1].amp], room), (b, js)
    rc, cli = parse("-b", "8", "--jam=cw,0,0")                  # 2047 + 250 > 2047
    assert rc == 0 and cli.impair.shift == 1
    rc, cli = parse("-b", "8", "--jam=cw,30,0")                 # 2047 + 7906 <= 2047 * 8
    assert rc == 0 and cli.impair.shift == 3
    rc, cli = parse("-b", "16", "--jam=cw,30,0")
    assert rc == 0 and cli.impair.shift == 0
    rc, cli = parse("-b", "1", "--jam=cw,42,0")
    assert rc == 0 and cli.impair.shift == 0
    rc, cli = parse("-b", "8", "--jam=cw,30,0", "--noise-shift=7")          # accepted with --jam
    assert rc == 0 and cli.impair.shift == 7 and cli.impair.sigma_q8 == 0
    rc, cli = parse("-b", "8", "--jam=cw,30,0", "--cn0=45", "--seed=9", "--noise-shift=auto")
    assert rc == 0 and cli.impair.seed == 9 and cli.impair.sigma_q8 > 0


@pytest.mark.parametrize("args", [
    ("--jam=",), ("--jam=cw",), ("--jam=cw,0",), ("--jam=cw,0,1,2",), ("--jam=tone,0,1",),
    ("--jam=cw,x,1",), ("--jam=cw,0,1x",), ("--jam=cw,nan,1",), ("--jam=cw,43,0",),
    ("--jam=cw,0,1300000",), ("--jam=cw,0,1,pulse",), ("--jam=cw,0,1,pulse,1e-3",),
    ("--jam=cw,0,1,gate,1e-3,0.5",), ("--jam=cw,0,1,pulse,1e-3,1.5",),
    ("--jam=cw,0,1,pulse,0,0.5",), ("--jam=cw,0,1,pulse,1e-3,0.5,7",),
    ("--jam=sweep,0,1,2",), ("--jam=sweep,0,1,2,0",), ("--jam=sweep,0,1,2,-1",),
    ("--jam=sweep,0,1,2,1e-9",), ("--jam=sweep,0,1,1300000,1e-3",),
    ("--jam=sweep,0,1,2,1e-3,pulse,1e-3",), ("--jam=cw,0,1", "--seed=3"),
    ("--jam=cw,0,1", "--noise-shift=9"), ("--jam=cw,0,1,",), ("--jam=cw,,1",),
])
def test_cli_jam_errors(args):
    rc, _ = parse("-b", "8", *args)
    assert rc == 1


def test_from_cli_sets_jam():
    scn, out = G.Scenario.from_cli(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1",
                                    "-s", "1000000", "-b", "8", "--jam=cw,30,0",
                                    "--jam=sweep,0,-400e3,400e3,137e-6", "-o", "x.bin"])
    assert out == "x.bin" and len(scn.jam) == 2 and scn.impair.sigma_q8 == 0
    assert as_dict(scn.jam[0]) == O.make(1e6, 30.0, 0.0)
    assert as_dict(scn.jam[1]) == O.make(1e6, 0.0, -400e3, 400e3, 137e-6)
    scn.close()
    scn, _ = G.Scenario.from_cli(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1"])
    assert scn.jam is None and scn.impair is None
    scn.close()


def test_run_node_refuses_jammers():
    from gpssim_amd.node import run_node
    with pytest.raises(ValueError, match="jam"):
        run_node(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1", "--jam=cw,0,0"], 0, 1, 0)


def test_struct_sizes_match_the_c_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpssim_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gss_jam_t), '
                   'sizeof(gss_cli_t), sizeof(gss_run_opts_t), offsetof(gss_cli_t, jam), '
                   'offsetof(gss_run_opts_t, jam), offsetof(gss_run_opts_t, n_jam));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == [C.sizeof(G.Jam), C.sizeof(G._Cli), C.sizeof(G._RunOpts), G._Cli.jam.offset,
                   G._RunOpts.jam.offset, G._RunOpts.n_jam.offset]
    assert got[0] == 48


# ---- gss_run on the CPU fakes ------------------------------------------------------------------
@pytest.fixture(scope="module")
def fake_build(tmp_path_factory):
    """jam_fake.cpp on the CPU fakes (tests/fake_build.py): with its launch, and without"""
    return programs(tmp_path_factory, "jam_fake")


def test_gss_run_jammed_on_fake_device(fake_build):
    r = subprocess.run([fake_build["jam_fake"], NAV], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "argument errors ok" in r.stdout and "all jammed runs ok" in r.stdout


def test_gss_run_refuses_jammers_without_a_launch(fake_build):
    r = subprocess.run([fake_build["jam_fake_nolaunch"], NAV], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "refused ok" in r.stdout and "jammer launch" in r.stdout


def test_jam_check_program(tmp_path):
    """tests/helpers/jam_check.c without the sanitizers (tools/jam_sanitize.sh runs it with them)"""
    hostdir = os.path.join(REPO, "gps-sdr-sim_amd", "csrc", "host")
    srcs = [os.path.join(hostdir, f) for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    exe = str(tmp_path / "jam_check")
    subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"), "-o",
                    exe] + srcs + [os.path.join(REPO, "tests", "helpers", "jam_check.c"), "-lm",
                                   "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "jam_check ok" in r.stdout, r.stdout[-4000:]


# ---- what the receiver sees --------------------------------------------------------------------
PHYS_SIGMA = int(np.floor(256 * 250 * np.sqrt(AO.PHYS_FS / (2 * 10 ** (AO.PHYS_CN0 / 10))) + 0.5))
# (name, jammer arguments of jam_make after fs, {fmt: shift}, found)
RECEIVER = [
    ("cw0", (0.0, 0.0), {16: 0, 8: 2}, True),
    ("cw30", (30.0, 0.0), {16: 0, 8: 5}, False),
    ("sweep0", (0.0, -400e3, 400e3, 137e-6), {16: 0, 8: 2}, True),
]


def receiver_verdict(peaks, blk, nch, found, noise=True):
    if found and noise:
        AO.check_physical(peaks, blk, nch, level=False, found=True)
    elif found:
        # Without noise the search has no Gaussian floor: the satellites' own cross-correlations
        # are the floor, and on the noise-free, jammer-free block itself they already take absent
        # PRNs over the threshold (PRN 5: 4.6 against 4.13).  The false-alarm half of
        # check_physical is therefore a statement about the noisy variant alone; here every
        # present satellite is located and over the threshold.
        AO.check_physical(peaks, blk, nch, level=False, found=False)
        by_prn = {int(p["prn"]): p for p in peaks}
        for row in blk[0][:nch[0]]:
            prn = G.acq_expect(row, AO.PHYS_FS, 0)["prn"]
            assert G.acq_ratio(by_prn[prn]) >= AO.phys_threshold(), prn
    else:
        ratios = [G.acq_ratio(p) for p in peaks]
        print("largest ratio %.2f against %.2f" % (max(ratios), AO.phys_threshold()))
        assert len(ratios) == 32 and max(ratios) < AO.phys_threshold()


@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("fmt", [16, 8])
@pytest.mark.parametrize("name,args,shifts,found", RECEIVER)
def test_receiver(name, args, shifts, found, fmt, noise):
    """a tone at the satellites' level leaves the eleven found; 30 dB above it nothing reaches
    the threshold; a sweep at their level (P = 137, which does not divide the 1 ms window) leaves
    them found.  With the fixture's noise (50 dB-Hz, seed 7) and without."""
    clean, blk, nch = AO.noisy_block(16, clean=True)
    j = G.jam_make(float(AO.PHYS_FS), *args)
    if name == "sweep0":
        assert j.sweep == 137
    imp = G.Impair(PHYS_SIGMA if noise else 0, shifts[fmt], 7)
    data = G.jam_host(imp, [j], clean.view(np.int16), 0, fmt)
    peaks, _, _ = G.acquire_host(AO.PHYS_ACQ(fmt), data)
    receiver_verdict(peaks, blk, nch, found, noise)
