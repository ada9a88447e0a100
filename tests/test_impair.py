"""Additive noise at a chosen C/N0 (include/gpssim_amd.h, gss_impair_t), the parts that need no
GPU: the half-normal table, the host statement gss_impair_host against the numpy restatement of
tests/impair_oracle.py byte for byte, the statistics of the draws, the command-line options, and
gss_run with the impairment on the CPU fakes of tests/helpers (impair_fake.cpp)."""
import ctypes as C
import os
import statistics
import subprocess

import numpy as np
import pytest

from conftest import NAV, REPO
from fake_build import programs

import gpssim_amd as G
import impair_oracle as O
from impair_oracle import SHIFTS, SIGMAS, SIZES, STARTS, samples


def test_philox_known_answers():
    O.check_known_answers()


def test_table():
    T = G.noise_table()
    nd = statistics.NormalDist()
    assert T.shape == (4097,)
    for i in range(4096):
        assert abs(int(T[i]) - 65536 * nd.inv_cdf(0.5 + i / 8192)) <= 1, i
    assert abs(int(T[4096]) - 65536 * nd.inv_cdf(1 - 1 / 32768)) <= 1
    assert (np.diff(T.astype(np.int64)) > 0).all()
    assert T[0] == 0 and T[4096] == 262719
    assert np.abs(T.astype(np.int64) - O.table()).max() <= 1


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_impair_host_equals_oracle(fmt):
    T_same = np.array_equal(G.noise_table().astype(np.int64), O.table())
    assert T_same, "the library's table differs from the oracle's: byte parity cannot hold"
    for n in SIZES[fmt]:
        iq = samples(n, seed=n)
        for sigma in SIGMAS:
            for shift in SHIFTS:
                for s0 in STARTS:
                    seed = (0x9E3779B97F4A7C15 * (s0 + 1) + sigma) & (2**64 - 1)
                    got = G.impair_host(G.Impair(sigma, shift, seed), iq, s0, fmt)
                    want = O.impair(seed, sigma, shift, iq, s0, fmt)
                    assert got.shape == want.shape == (G.impair_bytes(n, fmt),)
                    assert np.array_equal(got, want), (fmt, n, sigma, shift, s0)


def test_clamps_fire():
    """the grid's large sigmas reach both rails of SC16 and SC08"""
    iq = samples(7803)
    o16 = O.impair(1, 256 * 20000, 0, iq, 0, 16).view(np.int16)
    o8 = O.impair(1, 256 * 994, 0, iq, 0, 8).view(np.int8)
    assert o16.min() == -32768 and o16.max() == 32767
    assert o8.min() == -128 and o8.max() == 127


def test_impair_host_in_place_sc16():
    iq = samples(1001)
    imp = G.Impair(256 * 300, 1, 5)
    want = G.impair_host(imp, iq, 77, 16)
    buf = iq.copy()
    p = C.c_void_p(buf.ctypes.data)
    assert G.lib().gss_impair_host(C.byref(imp), p, 77, 1001, 16, p) == 0
    assert np.array_equal(buf.view(np.uint8), want)


def test_impair_host_argument_errors():
    iq = samples(8)
    out = np.zeros(64, np.uint8)
    pi, po = C.c_void_p(iq.ctypes.data), C.c_void_p(out.ctypes.data)
    f = G.lib().gss_impair_host
    assert f(C.byref(G.Impair(0x1000000, 0, 0)), pi, 0, 8, 16, po) == -1
    assert f(C.byref(G.Impair(1, 9, 0)), pi, 0, 8, 16, po) == -1
    assert f(C.byref(G.Impair(1, -1, 0)), pi, 0, 8, 16, po) == -1
    assert f(C.byref(G.Impair(1, 0, 0)), pi, 0, 8, 4, po) == -1
    assert f(C.byref(G.Impair(1, 0, 0)), pi, 0, 6, 1, po) == -1          # SC01: n % 4
    assert f(C.byref(G.Impair(1, 0, 0)), pi, 0, 8, 8, pi) == -1          # in place: SC16 only
    assert f(C.byref(G.Impair(1, 0, 0)), pi, 0, 8, 1, pi) == -1
    assert f(C.byref(G.Impair(1, 0, 0)), None, 0, 8, 16, po) == -1
    assert f(C.byref(G.Impair(1, 0, 0)), pi, 2**64 - 4, 8, 16, po) == -1
    assert f(C.byref(G.Impair(0xFFFFFF, 8, 0)), pi, 0, 8, 16, po) == 0


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_prefix_free(fmt):
    """impairing [a, b) then [b, c) is impairing [a, c): odd and even cuts"""
    imp = G.Impair(256 * 150, 2, 99)
    a, n = 2**32 - 40, 96
    iq = samples(n)
    whole = G.impair_host(imp, iq, a, fmt)
    for cut in ([33, 64] if fmt != 1 else [32, 64]):
        parts = np.concatenate([G.impair_host(imp, iq[:2 * cut], a, fmt),
                                G.impair_host(imp, iq[2 * cut:], a + cut, fmt)])
        assert np.array_equal(parts, whole), cut


def test_statistics():
    """2^20 draws (I and Q of 2^19 samples) at sigma = 1000 LSB.  The sampling errors: std
    0.07 %, mean 0.001 sigma, kurtosis 0.005, so the limits sit >= 10 standard errors out."""
    n, sigma = 1 << 19, 1000
    zero = np.zeros(2 * n, np.int16)
    g = G.impair_host(G.Impair(256 * sigma, 0, 2024), zero, 12345, 16).view(np.int16)
    g = g.astype(np.float64)
    assert len(g) == 1 << 20 and np.abs(g).max() < 32767           # 4.009 sigma: no clamp
    assert abs(g.std() / sigma - 1) <= 0.01
    assert abs(g.mean()) <= 0.01 * sigma
    k = ((g - g.mean()) ** 4).mean() / g.var() ** 2
    assert 2.9 <= k <= 3.1
    i, q = g[0::2], g[1::2]
    assert abs(np.corrcoef(i, q)[0, 1]) < 0.01 and abs(np.corrcoef(i[1:], i[:-1])[0, 1]) < 0.01


def parse(*args):
    cli = G._Cli()
    argv = [b"gps-sdr-sim", b"-e", NAV.encode()] + [a.encode() for a in args]
    arr = (C.c_char_p * len(argv))(*argv)
    return G.lib().gss_cli_parse(len(argv), arr, C.byref(cli)), cli


def test_cli_noise_options():
    rc, cli = parse("-s", "1000000", "-b", "16")
    assert rc == 0 and cli.has_impair == 0
    want = int(np.floor(256 * 250 * np.sqrt(1e6 / (2 * 10 ** 4.5)) + 0.5))
    assert abs(want / 256 - 994) < 1
    for b, shift in (("16", 0), ("8", 2), ("1", 0)):
        # the options before -s and -b: they are resolved after the whole line is read
        rc, cli = parse("--cn0=45", "-s", "1000000", "-b", b)
        assert rc == 0 and cli.has_impair == 1
        assert (cli.impair.sigma_q8, cli.impair.shift, cli.impair.seed) == (want, shift, 0)
        assert cli.opt.data_format == int(b) and cli.opt.samp_freq == 1e6
    rc, cli = parse("-b", "8", "--noise-sigma=12.5", "--seed=18446744073709551615",
                    "--noise-shift=7")
    assert rc == 0 and cli.has_impair == 1
    assert (cli.impair.sigma_q8, cli.impair.shift, cli.impair.seed) == (3200, 7, 2**64 - 1)
    rc, cli = parse("--noise-sigma=0", "--noise-shift=auto", "--seed=0x10")
    assert rc == 0 and (cli.impair.sigma_q8, cli.impair.shift, cli.impair.seed) == (0, 0, 16)
    rc, cli = parse("-b", "8", "--noise-sigma=65535")                 # no shift is enough: 8
    assert rc == 0 and cli.impair.shift == 8
    rc, cli = parse("-b", "16", "--noise-sigma=7680.1")               # 4 sigma + 2047 > 32767
    assert rc == 0 and cli.impair.shift == 1
    rc, cli = parse("-b", "16", "--noise-sigma=7680")
    assert rc == 0 and cli.impair.shift == 0


@pytest.mark.parametrize("args", [
    ("--cn0=45", "--noise-sigma=3"), ("--cn0=",), ("--cn0=abc",), ("--cn0=45x",), ("--cn0=nan",),
    ("--cn0=-300",), ("--noise-sigma=-1",), ("--noise-sigma=65536",), ("--noise-sigma=",),
    ("--cn0=45", "--noise-shift=9"), ("--cn0=45", "--noise-shift=-1"),
    ("--cn0=45", "--noise-shift=1.5"), ("--cn0=45", "--noise-shift=x"), ("--cn0=45", "--seed=-1"),
    ("--cn0=45", "--seed=18446744073709551616"), ("--cn0=45", "--seed=12q"),
    ("--cn0=45", "--seed="), ("--seed=3",), ("--noise-shift=2",),
])
def test_cli_noise_option_errors(args):
    rc, _ = parse("-b", "8", *args)
    assert rc == 1


def test_from_cli_sets_impair():
    scn, out = G.Scenario.from_cli(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1",
                                    "-s", "1000000", "-b", "8", "--cn0=45", "--seed=7",
                                    "-o", "x.bin"])
    assert out == "x.bin" and scn.impair.seed == 7 and scn.impair.shift == 2
    scn.close()
    scn, _ = G.Scenario.from_cli(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1"])
    assert scn.impair is None
    scn.close()


def test_run_node_refuses_noise_options():
    from gpssim_amd.node import run_node
    with pytest.raises(ValueError, match="noise"):
        run_node(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1", "--cn0=45"], 0, 1, 0)


@pytest.fixture(scope="module")
def fake_build(tmp_path_factory):
    """impair_fake.cpp on the CPU fakes (tests/fake_build.py): with its launch, and without"""
    return programs(tmp_path_factory, "impair_fake")


def test_gss_run_impaired_on_fake_device(fake_build):
    r = subprocess.run([fake_build["impair_fake"], NAV], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all impaired runs ok" in r.stdout


def test_gss_run_refuses_noise_without_a_launch(fake_build):
    r = subprocess.run([fake_build["impair_fake_nolaunch"], NAV], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "refused ok" in r.stdout and "impairment launch" in r.stdout


def test_stage_split_check_program(tmp_path):
    """tests/helpers/stage_split_check.c: the head/groups split the stages' launches share
    (csrc/common/gss_stage.h), by its properties over every format, offset and small n, with
    gss_fmt_bytes, gss_stage_grid and gss_imp_put"""
    exe = str(tmp_path / "stage_split_check")
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(REPO, "tests", "helpers", "stage_split_check.c")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "stage_split_check ok" in r.stdout, r.stdout[-4000:]
