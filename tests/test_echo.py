"""Multipath echoes (include/gpssim_amd.h, gss_echo_t), the parts that need no GPU: the host
statement gss_echo_host against the restatement of tests/echo_oracle.py byte for byte,
gss_echo_make against its formulas, an echo with no delay against the render itself, the
code-phase bias an echo gives a tracking loop against the multipath error envelope, the
command-line option, and gss_run with echoes on the CPU fakes of tests/helpers (echo_fake.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import NAV, REPO
from fake_build import programs

import gpssim_amd as G
import echo_oracle as O
import oracle
from jam_oracle import tables

CASES = O.cases_cached()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_echo_host_equals_oracle(i):
    got = O.run_host(CASES[i])
    assert got.dtype == np.int16 and np.array_equal(got, O.want(i)), CASES[i][0]


def test_cases_cover_what_they_claim():
    """counted over the pairs that reach a sample (live, gain not 0): 64 of them in a block, every
    delay of DELAYS, every start of STARTS with a dstep of either sign, every block length, delays
    reaching before the frame, code past word 59, carr0 == 1.0; besides, a PRN no row has, a
    silent echo, rows out of range, zero and negative gains, steps above one chip, both clamps"""
    pairs, before, past, one, silent, bad = 0, 0, 0, 0, 0, 0
    delays, starts, sizes = set(), set(), set()
    for _, es, blk, nch, nav, n, s0, iq in CASES:
        for b in range(len(nch)):
            rows = blk[b, :nch[b]]
            pairs = max(pairs, sum(O.contributes(e, r, 32, len(nav)) for e in es for r in rows))
            bad += sum(not O.in_range(r) for r in rows)
            for e in es:
                assert not any(e["prn"] == O.NO_PRN and O.live(e, r, 32, len(nav)) for r in rows)
                for r in rows:
                    silent += O.live(e, r, 32, len(nav)) and e["alpha_q16"] == 0
                    if not O.contributes(e, r, 32, len(nav)):
                        continue
                    P0, Ps, X0, Cs, g = O.ints(e, r)
                    delays.add(e["delay"])
                    sizes.add(n)
                    if e["dstep"]:
                        starts.add((s0, e["dstep"] >> 63))
                    before += X0 < 0
                    past += ((X0 + (n - 1) * Cs) >> 32) // 1023 // 600 > 59
                    one += float(r["carr0"]) == 1.0
    assert pairs == 64 and before > 0 and past > 0 and one > 0 and silent > 0 and bad >= 11
    assert delays == set(O.DELAYS) and sizes == set(O.SIZES)
    assert starts == {(s0, sign) for s0 in O.STARTS for sign in (0, 1)}
    gains = {int(r["gain"]) for c in CASES for b in range(len(c[3])) for r in c[2][b, :c[3][b]]}
    assert 0 in gains and min(gains) < 0 and max(float(s) for s in O.X.CODE_STEPS) > 1000
    i = [c[0] for c in CASES].index("clamp_a%d" % (1 << 18))
    v = O.want(i)
    assert (v == 32767).sum() > 10 and (v == -32768).sum() > 10
    e, blk = CASES[i][1][0], CASES[i][2]
    assert abs(O.ints(e, blk[0, 0])[4]) == 32767


def test_ranges_compose():
    """blocks split at any block boundary, sample0 moved accordingly, give the whole"""
    name, es, blk, nch, nav, n, s0, iq = next(c for c in CASES if c[5] == 33 and len(c[1]) == 4)
    echoes = [O.to_echo(e) for e in es]
    whole = G.echo_host(echoes, blk, nch, O.ca_table(), nav, n, s0, iq)
    for cut in range(len(nch) + 1):
        a = G.echo_host(echoes, blk[:cut], nch[:cut], O.ca_table(), nav, n, s0, iq[:2 * cut * n])
        b = G.echo_host(echoes, blk[cut:], nch[cut:], O.ca_table(), nav, n, s0 + cut * n,
                        iq[2 * cut * n:])
        assert np.array_equal(np.concatenate([a, b]), whole), cut


def test_no_echo_and_empty_blocks_change_nothing():
    name, es, blk, nch, nav, n, s0, iq = next(c for c in CASES if c[5] == 1025 and len(c[1]) == 4)
    assert np.array_equal(G.echo_host([], blk, nch, O.ca_table(), nav, n, s0, iq), iq)
    got = G.echo_host([O.to_echo(e) for e in es], blk, np.zeros_like(nch), O.ca_table(), nav, n, s0,
                      iq)
    assert np.array_equal(got, iq)


BAD_ECHOES = [dict(delay=O.DELAY_END), dict(alpha_q16=(1 << 18) + 1), dict(prn=-1), dict(prn=33)]


def test_echo_host_argument_errors():
    """every refusal leaves the buffer untouched"""
    blk, nch, nav = O.case(8, [2, 1], seed=1)
    ca = O.ca_table()
    iq = np.full(2 * 16, 0x5A5A, np.int16)
    f = G.lib().gss_echo_host
    P = lambda a: C.c_void_p(a.ctypes.data)
    args = lambda arr, ne, nb=2, n=8, nca=32, nnav=len(nav), s0=0, nchp=nch: (
        arr, ne, P(blk), P(nchp), nb, n, P(ca), nca, P(nav), nnav, s0, P(iq))
    good = (G.Echo * 5)(*[G.Echo(delay=O.DELAY_END - 1, alpha_q16=1 << 18, prn=32)] * 5)
    assert f(*args(good, 4)) == 0
    assert (iq == 0x5A5A).all()                        # PRN 32: no row of these
    for bad in BAD_ECHOES:
        arr = (G.Echo * 2)(G.Echo(), G.Echo(**bad))
        assert f(*args(arr, 2)) == -1, bad
    assert G.lib().gss_echo_check(good, 4) == 0
    assert G.lib().gss_echo_check(good, 5) == -1 and G.lib().gss_echo_check(None, 1) == -1
    one = (G.Echo * 1)(G.Echo())
    assert f(*args(one, 5)) == -1 and f(*args(one, -1)) == -1 and f(*args(None, 1)) == -1
    assert f(*args(one, 1, n=0)) == -1 and f(*args(one, 1, nb=-1)) == -1
    assert f(*args(one, 1, nca=0)) == -1 and f(*args(one, 1, nnav=0)) == -1
    assert f(*args(one, 1, s0=2 ** 64 - 15)) == -1
    assert f(*args(one, 1, nchp=np.array([2, 17], np.int32))) == -1
    assert f(*args(one, 1, nchp=np.array([-1, 1], np.int32))) == -1
    assert (iq == 0x5A5A).all()
    with pytest.raises(G.GssError) as e:
        G.echo_host([G.Echo()] * 5, blk, nch, ca, nav, 8, 0, iq)
    assert e.value.code == -1


MAKE = [(1e6, 0, 150.0, 6.0), (2.6e6, 7, 0.0, 0.0, 0.0, 0.0), (2.6e6, 32, 146.5261280547409, 6.0206),
        (1e6, 1, 299000.0, -12.0, 180.0, -0.5), (1e6, 3, 1.0, 3.0, -90.0, 499999.0),
        (1000010.0, 0, 29.3, 200.0, 720.0, -499999.0), (1e6, 5, 10.0, 1.0, -1e-20, 1e-9),
        (1e6, 5, 10.0, 1.0, 359.99999999999994, 0.0)]


@pytest.mark.parametrize("args", MAKE)
def test_echo_make(args):
    got, want = G.echo_make(*args), O.make(*args)
    assert {k: getattr(got, k) for k in want} == want


@pytest.mark.parametrize("args", [
    (1e6, 33, 1.0, 0.0), (1e6, -1, 1.0, 0.0), (1e6, 1, -1.0, 0.0), (1e6, 1, 299792.458, 0.0),
    (1e6, 1, 1.0, -12.1), (1e6, 1, 1.0, 0.0, 0.0, 500e3), (1e6, 1, 1.0, 0.0, 0.0, -500e3),
    (0.0, 1, 1.0, 0.0), (float("nan"), 1, 1.0, 0.0), (1e6, 1, float("nan"), 0.0),
    (1e6, 1, 1.0, float("inf")), (1e6, 1, 1.0, 0.0, float("nan"), 0.0),
    (1e6, 1, 1.0, 0.0, 0.0, float("inf")),
])
def test_echo_make_rejections(args):
    with pytest.raises(G.GssError) as e:
        G.echo_make(*args)
    assert e.value.code == -1


# ---- an echo with no delay is the direct signal -------------------------------------------------
def one_channel(fs, n, nblk, doppler_hz=1500.0, code_step=None, seed=3):
    """(blk, nch, nav) of one satellite (PRN 1, gain 128) over nblk consecutive blocks of n samples:
    every block's row continues the block before it exactly (the reference's own recurrences)"""
    rng = np.random.default_rng(seed)
    nav = rng.integers(0, 1 << 30, size=(1, G.NAV_WORDS), dtype=np.uint32)
    blk = np.zeros((nblk, G.MAXCH), G.CHAN_DTYPE)
    cs = (1.023e6 + doppler_hz / 1540.0) / fs if code_step is None else code_step
    carr, code, cnt = 0.123456789, 0.0, (0, 0, 0)      # a phase that lands on no table-cell boundary
    for b in range(nblk):
        p = blk[b, 0]
        p["carr0"], p["carr_step"], p["code0"], p["code_step"] = carr, doppler_hz / fs, code, cs
        p["icode"], p["ibit"], p["iword"] = cnt
        p["gain"], p["ca_tbl"], p["nav_tbl"] = 128, 0, 0
        carr = oracle.carr_brute(carr, doppler_hz / fs, n)
        code, *cnt = oracle.code_brute(code, cs, n, *cnt)
    return blk, np.ones(nblk, np.int32), nav


@pytest.mark.parametrize("fs,n", [(2.6e6, 260000), (1e6, 100000)])
def test_an_echo_without_delay_is_the_render(fs, n):
    """added to zeros, an echo with delay 0, alpha 1 and no phase terms is the reference's render
    of its channel except where the Q32 code step or the exact carrier puts a sample across a
    chip or cell boundary: at most 16 samples of the block (the definition alone gave 0 to 2),
    each the neighbouring chip's sign or the neighbouring table cell.  (A start phase of 0.25 at
    1500 Hz and 2.6 MS/s puts every 325th sample exactly on a cell boundary, where the reference's
    rounded recurrence falls on either side and the integers always below: 798 samples, all of
    them the neighbouring cell.  one_channel() starts at a phase that meets no boundary.)"""
    cos, sin = tables()
    for dop in (1500.0, -3200.0, 0.0, 4999.0):
        blk, nch, nav = one_channel(fs, n, 1, dop, code_step=0.3935)
        out, rc = oracle.synth(blk, nch, O.ca_table(), nav, n, 16)
        assert rc == 0
        x = out.view(np.int16).reshape(-1, 2).astype(np.int64)
        y = G.echo_host([G.Echo(prn=1)], blk, nch, O.ca_table(), nav, n, 0,
                        np.zeros(2 * n, np.int16)).reshape(-1, 2).astype(np.int64)
        diff = np.flatnonzero((x != y).any(axis=1))
        print("fs %.0f doppler %.0f: %d of %d samples differ" % (fs, dop, len(diff), n))
        assert len(diff) <= 16
        cells = {(int(s * cos[j]), int(s * sin[j])): (s, j) for j in range(512) for s in (1, -1)}
        for i in diff:
            if np.array_equal(y[i], -x[i]):                        # the neighbouring chip
                continue
            (sx, jx), (sy, jy) = cells[tuple(x[i])], cells[tuple(y[i])]
            assert sx == sy and (jx - jy) % 512 in (1, 511), (i, x[i], y[i])


# ---- physics: the bias of the tracked code phase ------------------------------------------------
PHYS_FS, PHYS_N, PHYS_BLOCKS, PHYS_DOPPLER = 2600000, 260000, 25, 1500.0


@pytest.fixture(scope="module")
def phys():
    """the direct signal of one satellite (gain 128, Doppler 1500 Hz, no noise) over 2.5 s, its
    rows, and the code phase a default tracking loop gives every 1 ms from 1 s on"""
    blk, nch, nav = one_channel(float(PHYS_FS), PHYS_N, PHYS_BLOCKS, PHYS_DOPPLER)
    out, rc = oracle.synth(blk, nch, O.ca_table(), nav, PHYS_N, 16)
    assert rc == 0
    iq = out.view(np.int16)

    def code_of(iq):
        jobs = np.zeros(1, G.TRK_JOB_DTYPE)
        n_epoch = 2450
        jobs[0] = (0, 1, int(round(PHYS_DOPPLER / PHYS_FS * 2 ** 32)), n_epoch, 0)
        rec, count = G.track_host(G.Trk(PHYS_FS, 16), iq, jobs)
        assert count[0] == n_epoch                     # the run keeps all its epochs
        obs = G.observables_host(PHYS_FS, rec, count, PHYS_FS, 2600, 1400)
        assert (obs["epoch"] >= 0).all()
        return obs[0]["code"].astype(np.int64)

    return blk, nch, nav, iq, code_of, code_of(iq)


def bias(phys, echo):
    blk, nch, nav, iq, code_of, ref = phys
    got = code_of(G.echo_host([echo], blk, nch, O.ca_table(), nav, PHYS_N, 0, iq))
    M = 1023 << 32
    d = ((got - ref + M // 2) % M - M // 2) / 2.0 ** 32
    print("bias %+.5f chip, spread %.5f over %d instants" % (d.mean(), d.std(), len(d)))
    return d


@pytest.mark.parametrize("delay,theta0,want", [(1 << 31, 0, -1.0 / 6), (1 << 30, 0, -1.0 / 12),
                                               (1 << 31, 1 << 63, 0.2)])
def test_code_bias_follows_the_multipath_envelope(phys, delay, theta0, want):
    """early-late spacing 1 chip, alpha 1/2: in phase the DLL's zero moves by alpha tau / (1 +
    alpha) chips late; in anti-phase by the zero of |E| - |L| with triangle correlations, 0.5 - b
    = 1.5 b.  The bound is six times the spread over the instants (0.0015)."""
    d = bias(phys, G.Echo(delay=delay, theta0=theta0, alpha_q16=32768, prn=1))
    assert abs(d.mean() - want) <= 0.01


def test_code_bias_of_a_silent_echo_is_zero(phys):
    d = bias(phys, G.Echo(delay=1 << 31, alpha_q16=0, prn=1))
    assert (d == 0).all()


# ---- the command line --------------------------------------------------------------------------
def parse(*args):
    cli = G._Cli()
    argv = [b"gps-sdr-sim", b"-e", NAV.encode()] + [a.encode() for a in args]
    arr = (C.c_char_p * len(argv))(*argv)
    return G.lib().gss_cli_parse(len(argv), arr, C.byref(cli)), cli


def as_dict(e):
    return {k: getattr(e, k) for k in O.E()}


def test_cli_multipath_forms():
    fs = 1e6
    rc, cli = parse("-s", "1000000", "-b", "16")
    assert rc == 0 and cli.n_echo == 0 and cli.has_impair == 0
    forms = [("all,150,6", (0, 150.0, 6.0)), ("7,40.5,3,180", (7, 40.5, 3.0, 180.0)),
             ("32,0,0,-90,2.5", (32, 0.0, 0.0, -90.0, 2.5)), ("1,1e3,-12,0,-1e3", (1, 1e3, -12.0, 0.0, -1e3))]
    for text, args in forms:                 # the option before -s: resolved at the run's rate
        rc, cli = parse("--multipath=" + text, "-s", "1000000", "-b", "8")
        assert rc == 0 and cli.n_echo == 1 and cli.n_jam == 0 and cli.has_impair == 1, text
        assert as_dict(cli.echo[0]) == O.make(fs, *args), text
        assert (cli.impair.sigma_q8, cli.impair.seed) == (0, 0)
    rc, cli = parse("-s", "1000000", *["--multipath=" + t for t, _ in forms], "--jam=cw,0,0")
    assert rc == 0 and cli.n_echo == 4 and cli.n_jam == 1
    for i, (_, args) in enumerate(forms):
        assert as_dict(cli.echo[i]) == O.make(fs, *args)
    rc, cli = parse("-s", "1000000", *["--multipath=" + t for t, _ in forms], "--multipath=all,1,1")
    assert rc == 1


def auto_shift(sigma_q8, amps, alphas, room):
    peak = 4.0 * (sigma_q8 / 256.0) + 2047.0 + sum(a * 250.0 / 65536.0 for a in amps)
    peak += sum(2047.0 * a / 65536.0 for a in alphas)
    return min(s for s in range(9) if peak <= room * 2**s or s == 8)


def test_cli_auto_shift_with_an_echo():
    for b, room in (("16", 32767.0), ("8", 2047.0)):
        for db in ("0", "6", "-12", "40"):
            rc, cli = parse("-s", "1000000", "-b", b, "--multipath=all,150," + db)
            assert rc == 0 and cli.impair.sigma_q8 == 0
            assert cli.impair.shift == auto_shift(0, [], [cli.echo[0].alpha_q16], room), (b, db)
            rc, cli = parse("-s", "1000000", "-b", b, "--cn0=45", "--multipath=all,150," + db,
                            "--multipath=3,10,0", "--jam=cw,10,1000")
            assert rc == 0 and cli.n_echo == 2 and cli.n_jam == 1
            assert cli.impair.shift == auto_shift(
                cli.impair.sigma_q8, [cli.jam[0].amp],
                [cli.echo[0].alpha_q16, cli.echo[1].alpha_q16], room), (b, db)
    rc, cli = parse("-b", "8", "--multipath=all,150,6")         # 2047 + 1023.5 > 2047
    assert rc == 0 and cli.impair.shift == 1
    rc, cli = parse("-b", "8", "--multipath=all,150,-12")       # 2047 + 8149 <= 2047 * 8
    assert rc == 0 and cli.impair.shift == 3
    rc, cli = parse("-b", "16", "--multipath=all,150,-12")
    assert rc == 0 and cli.impair.shift == 0
    rc, cli = parse("-b", "1", "--multipath=all,150,-12")
    assert rc == 0 and cli.impair.shift == 0
    rc, cli = parse("-b", "8", "--multipath=all,150,6", "--noise-shift=7")
    assert rc == 0 and cli.impair.shift == 7 and cli.impair.sigma_q8 == 0


@pytest.mark.parametrize("args", [
    ("--multipath=",), ("--multipath=all",), ("--multipath=all,1",), ("--multipath=all,1,2,3,4,5",),
    ("--multipath=0,1,2",), ("--multipath=33,1,2",), ("--multipath=1.5,1,2",),
    ("--multipath=any,1,2",), ("--multipath=all,x,2",), ("--multipath=all,1,2x",),
    ("--multipath=all,nan,2",), ("--multipath=all,-1,2",), ("--multipath=all,3e5,2",),
    ("--multipath=all,1,-13",), ("--multipath=all,1,2,inf",), ("--multipath=all,1,2,0,1300000",),
    ("--multipath=all,1,2,",), ("--multipath=all,,2",), ("--multipath=all,1,2", "--seed=3"),
    ("--multipath=all,1,2", "--noise-shift=9"),
])
def test_cli_multipath_errors(args):
    rc, _ = parse("-b", "8", *args)
    assert rc == 1


def test_from_cli_sets_echo():
    scn, out = G.Scenario.from_cli(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1",
                                    "-s", "1000000", "-b", "8", "--multipath=all,150,6",
                                    "--multipath=7,40,3,180,2.5", "-o", "x.bin"])
    assert out == "x.bin" and len(scn.echo) == 2 and scn.jam is None and scn.impair.sigma_q8 == 0
    assert as_dict(scn.echo[0]) == O.make(1e6, 0, 150.0, 6.0)
    assert as_dict(scn.echo[1]) == O.make(1e6, 7, 40.0, 3.0, 180.0, 2.5)
    scn.close()
    scn, _ = G.Scenario.from_cli(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1"])
    assert scn.echo is None and scn.impair is None
    scn.close()


def test_run_node_refuses_echoes():
    from gpssim_amd.node import run_node
    with pytest.raises(ValueError, match="multipath"):
        run_node(["-e", NAV, "-l", "30.286502,120.032669,100", "-d", "1", "--multipath=all,150,6"],
                 0, 1, 0)


def test_cli_prints_one_line_per_echo(tmp_path):
    """the tool's stderr line per echo; they come before the device is opened, so they are there
    with and without a GPU"""
    exe = os.path.join(REPO, "gps-sdr-sim_amd", "bin", "gps-sdr-sim")
    r = subprocess.run([exe, "-e", NAV, "-l", "30.286502,120.032669,100", "-d", "0.3", "-s",
                        "1000000", "-b", "8", "-o", str(tmp_path / "x.bin"), "--multipath=all,150,6",
                        "--multipath=7,40,3,180"], capture_output=True, text=True, timeout=600)
    want = [O.make(1e6, 0, 150.0, 6.0), O.make(1e6, 7, 40.0, 3.0, 180.0)]
    for i, e in enumerate(want):
        line = ("Echo %d: prn = %d, delay = %d, alpha_q16 = %d, theta0 = %d, dstep = %d"
                % (i, e["prn"], e["delay"], e["alpha_q16"], e["theta0"], e["dstep"]))
        assert line in r.stderr, r.stderr[-2000:]


def test_struct_sizes_match_the_c_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpssim_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gss_echo_t), '
                   'sizeof(gss_cli_t), sizeof(gss_run_opts_t), offsetof(gss_cli_t, echo), '
                   'offsetof(gss_cli_t, n_echo), offsetof(gss_run_opts_t, echo), '
                   'offsetof(gss_run_opts_t, n_echo));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == [C.sizeof(G.Echo), C.sizeof(G._Cli), C.sizeof(G._RunOpts), G._Cli.echo.offset,
                   G._Cli.n_echo.offset, G._RunOpts.echo.offset, G._RunOpts.n_echo.offset]
    assert got[0] == 32


# ---- gss_run on the CPU fakes ------------------------------------------------------------------
@pytest.fixture(scope="module")
def fake_build(tmp_path_factory):
    """echo_fake.cpp on the CPU fakes (tests/fake_build.py): with its launch, and without"""
    return programs(tmp_path_factory, "echo_fake")


def test_gss_run_echoed_on_fake_device(fake_build):
    r = subprocess.run([fake_build["echo_fake"], NAV], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "argument errors ok" in r.stdout and "all echoed runs ok" in r.stdout


def test_gss_run_refuses_echoes_without_a_launch(fake_build):
    r = subprocess.run([fake_build["echo_fake_nolaunch"], NAV], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "refused ok" in r.stdout and "echo launch" in r.stdout


def test_echo_check_program(tmp_path):
    """tests/helpers/echo_check.c without the sanitizers (tools/echo_sanitize.sh runs it with them)"""
    hostdir = os.path.join(REPO, "gps-sdr-sim_amd", "csrc", "host")
    srcs = [os.path.join(hostdir, f) for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    exe = str(tmp_path / "echo_check")
    subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"), "-o",
                    exe] + srcs + [os.path.join(REPO, "tests", "helpers", "echo_check.c"), "-lm",
                                   "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "echo_check ok" in r.stdout, r.stdout[-4000:]
