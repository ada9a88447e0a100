"""Observables, navigation data and position fixes on the host (csrc/host/obs.c, navdata.c,
pvt.c): gss_obs_host against the restatement of tests/obs_oracle.py, byte for byte;
the ephemeris and ionosphere decoded from the simulator's own nav rows against the RINEX file;
the solver on observables built from truth; and the physical test: the static scenario is
tracked through noise, and the fixes come out at its location and start time."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import obs_oracle as B
import trk_oracle as O

C_LIGHT = 2.99792458e8


def host_equals(name):
    c = B.case(name)
    for g, grid in enumerate(c["grids"]):
        obs = G.observables_host(c["fs"], c["rec"], c["count"], *grid, threads=3)
        B.same(obs, B.want(name, g))


@pytest.mark.parametrize("name", B.NAMES)
def test_obs_host_equals_oracle(name):
    host_equals(name)


def test_the_counts_reach_the_edges():
    """every unit of the kernel's scan (a lane's records, a row's, a wave's, a workgroup's tile)
    minus one, exact and plus one, and two tiles plus one: a change of the kernel's constants
    must change these with it (csrc/hip/gss_obs.hip: OBS_ITEMS, OBS_THREADS)"""
    src = open(G.PKG_DIR + "/csrc/hip/gss_obs.hip").read()
    assert f"OBS_ITEMS = {B.LANE};" in src and f"OBS_THREADS = {B.TILE // B.LANE};" in src
    assert (B.LANE, B.ROW, B.WAVE, B.TILE) == (4, 64, 256, 1024)
    for u in (B.LANE, B.ROW, B.WAVE, B.TILE):
        assert {u - 1, u, u + 1} <= set(B.EDGE_COUNTS), u
    assert {0, 1, 2, 2 * B.TILE + 1} <= set(B.EDGE_COUNTS)
    c = B.case("edges")
    assert tuple(c["count"]) == B.EDGE_COUNTS and c["rec"].shape[1] > max(B.EDGE_COUNTS)
    # the first grid puts an instant into every epoch of every job
    w = B.want("edges", 0)
    for j, n in enumerate(c["count"]):
        assert set(w["epoch"][j]) - {-1} == set(range(n)), j
    big = B.case("big")
    assert len(big["count"]) == B.BIG_JOBS > 256 and sorted(set(big["count"])) == [3, B.BIG]
    assert B.BIG > 60 * B.TILE


def test_the_small_case_holds_every_kind_of_instant():
    c = B.case("small")
    rec, count = c["rec"], c["count"]
    assert list(count) == [0, 1, 2, 7] and rec.shape[1] > 7
    w0, w1, w2 = B.want("small", 0), B.want("small", 1), B.want("small", 2)
    assert (w0["epoch"][0] == -1).all()                          # count 0
    assert list(w0["epoch"][1][:3]) == [-1, -1, 0]               # before s_0, at s_0
    s1 = int(rec["s"][3, 1])
    assert list(w1["epoch"][3]) == [0, 0, 0, 1, 1, 1]            # s_e + n_e - 1, then s_(e+1)
    assert w1["code"][3][3] < w1["code"][3][2]                   # the code phase starts again
    for j in (1, 2, 3):                                          # the end of the last epoch
        e = w2["epoch"][j]
        last = int(np.flatnonzero(e >= 0)[-1])
        assert e[last] == count[j] - 1 and (e[last + 1:] == -1).all() and last + 1 < len(e)
        cs = O.cs_nominal(c["fs"]) + int(rec["dcs"][j, count[j] - 1])
        assert w2["code"][j][last] < B.M <= w2["code"][j][last] + cs
    assert s1 > 40 and (B.want("small", 4)["epoch"][:, 1] == -1).all()   # a step past the job
    assert B.want("small", 5).shape == (4, 0)


def test_adr_wraps():
    """at the ends of w the accumulated carrier passes 2^63 once the records span 2^32 samples.
    The tracking oracle's feedback and ends cases hold those w, but 40 epochs of them stay far
    below 2^63 (2^31 x 40 x 5122 < 2^49); the records 2^40 samples apart reach it."""
    w = B.want("jumps", 0)
    c = B.case("jumps")
    for j, step in enumerate((-2**31, 2**31 - 1)):
        ok = w["epoch"][j] >= 0
        t = np.array([(k << 39) - 5 for k in range(w.shape[1])], dtype=object)
        exact = [int(x) * step for x in t[ok]]
        assert max(abs(x) for x in exact) > 2**63
        assert [B.s64(x) for x in exact] == [int(x) for x in w["adr"][j][ok]]
    f = B.case("feedback_64000_wrap")
    assert {-2**31, 2**31 - 1} <= set(int(x) for x in f["rec"]["w"][:, 0])
    assert max(np.abs(np.diff(O.lengths(O.case("feedback_64000_maxkd"), j))).max()
               for j in range(3)) > 1


def test_obs_arguments():
    c = B.case("small")
    for bad in [(0, 0, 3), (0, 1, -1), (2**61 + 1, 1, 1), (0, 2**61, 4)]:
        with pytest.raises(G.GssError):
            G.observables_host(c["fs"], c["rec"], c["count"], *bad)
    with pytest.raises(G.GssError):
        G.observables_host(c["fs"], c["rec"], [0, 1, 2, 10], 0, 1, 1)       # count > pitch
    with pytest.raises(G.GssError):
        G.observables_host(999, c["rec"], c["count"], 0, 1, 1)


# ---- navigation data -------------------------------------------------------------------------
PI = 3.1415926535898
LSB = dict(toc=16.0, toe=16.0, af0=2.0**-31, af1=2.0**-43, af2=2.0**-55, tgd=2.0**-31,
           crs=2.0**-5, crc=2.0**-5, deltan=2.0**-43 * PI, m0=2.0**-31 * PI, cuc=2.0**-29,
           cus=2.0**-29, cic=2.0**-29, cis=2.0**-29, ecc=2.0**-33, sqrta=2.0**-19,
           omg0=2.0**-31 * PI, inc0=2.0**-31 * PI, aop=2.0**-31 * PI, omgdot=2.0**-43 * PI,
           idot=2.0**-43 * PI)
IONO_LSB = dict(alpha0=2.0**-30, alpha1=2.0**-27, alpha2=2.0**-24, alpha3=2.0**-24,
                beta0=2048.0, beta1=16384.0, beta2=65536.0, beta3=65536.0)


def row_subframes(words):
    """the five subframes of a nav row's frame (words 10..59) as NAV_SF_DTYPE"""
    sf = np.zeros(5, G.NAV_SF_DTYPE)
    for k in range(5):
        sf[k]["word"] = words[10 + 10 * k:20 + 10 * k]
        sf[k]["id"] = k + 1
        sf[k]["tow"] = int(words[11 + 10 * k]) >> 13 & 0x1FFFF
        sf[k]["epoch"] = 6000 * k
    return sf


def steady_rows():
    """{prn: its nav row's 60 words} of the static scenario's steady channels"""
    blk, nch, nav, _ = O.phys_rows()
    return {prn: nav[blk[0][k]["nav_tbl"]] for prn, k in O.steady_channels(blk, nch).items()}


def test_ephemeris_decoding():
    rows = steady_rows()
    assert len(rows) >= 8
    for prn, words in rows.items():
        sf = row_subframes(words)
        assert [int(w) >> 8 & 7 for w in words[11:60:10]] == [1, 2, 3, 4, 5]
        dec, rin = G.NavData(), G.NavData(NAV)
        assert rin.get(prn)["valid"] == 0
        for k in (2, 0):
            dec.add_subframe(prn, sf[k])
            assert dec.get(prn)["valid"] == 0, "two subframes do not make a set"
        dec.add_subframe(prn, sf[1])
        rin.add_subframe(prn, sf[1])                       # subframe 2 alone selects by IODE
        d, r = dec.get(prn), rin.get(prn)
        assert d["valid"] == 1 and r["valid"] == 1
        assert d["iode"] == r["iode"] and d["iodc"] == r["iodc"]
        for f, lsb in LSB.items():
            assert abs(d[f] - r[f]) <= lsb, (prn, f, d[f], r[f])
        rin3 = G.NavData(NAV)
        rin3.add_subframe(prn, sf[2])                      # ... and so does subframe 3
        assert rin3.get(prn) == r
        dec.add_subframe(prn, sf[3])                       # page 18
        d, r = dec.get(prn), rin.get(prn)
        assert d["iono_valid"] == 1 and r["iono_valid"] == 1
        for f, lsb in IONO_LSB.items():
            assert abs(d[f] - r[f]) <= lsb, (prn, f, d[f], r[f])
        for h in (dec, rin, rin3):
            h.close()


def test_a_foreign_iode_completes_nothing():
    prn, words = sorted(steady_rows().items())[0]
    sf = row_subframes(words)
    sf[2]["word"][9] ^= 1 << 22                            # the lowest bit of subframe 3's IODE
    dec, rin = G.NavData(), G.NavData(NAV)
    for k in (0, 1, 2):
        dec.add_subframe(prn, sf[k])
    rin.add_subframe(prn, sf[2])
    assert dec.get(prn)["valid"] == 0 and rin.get(prn)["valid"] == 0
    dec.add_subframe(prn, row_subframes(words)[2])
    assert dec.get(prn)["valid"] == 1
    with pytest.raises(G.GssError):
        dec.add_subframe(33, sf[0])


# ---- the solver on exact inputs --------------------------------------------------------------
def llh_to_ecef(lat_deg, lon_deg, h):
    a, e = 6378137.0, 0.0818191908426
    lat, lon = lat_deg / 57.2957795131, lon_deg / 57.2957795131
    n = a / np.sqrt(1 - (e * np.sin(lat)) ** 2)
    return np.array([(n + h) * np.cos(lat) * np.cos(lon), (n + h) * np.cos(lat) * np.sin(lon),
                     ((1 - e * e) * n + h) * np.sin(lat)])


def start_time():
    s = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=1e6)
    g0 = (s.start_week, s.start_sec)
    s.close()
    return g0


def exact_sats(nd, prns, g0, xyz, fs, t, no_iono=False):
    """PVT_SAT_DTYPE of the observables a perfect receiver at xyz whose sample 0 is at g0 reads at
    sample t: the transmit time g0 + t / fs - range / c in exact rationals, cut into the TOW count
    of the subframe it lies in, whole code periods since, and the code phase rounded to 2^-32
    chip (an error of at most 2^-33 chip = 1.1e-16 s)"""
    sats = np.zeros(len(prns), G.PVT_SAT_DTYPE)
    for i, prn in enumerate(prns):
        rx = Fraction(g0[1]) + Fraction(t) / Fraction(fs)
        rng, _ = nd.range(prn, g0[0], float(rx), xyz, no_iono)
        tx = rx - Fraction(rng) / Fraction(C_LIGHT)
        sub = tx // 6
        ms = (tx - 6 * sub) * 1000
        e = ms.numerator // ms.denominator
        code = round((ms - e) * B.M)
        if code == B.M:
            e, code = e + 1, 0
        sats[i]["prn"], sats[i]["sf_tow"], sats[i]["sf_epoch"] = prn, int(sub) + 1, 1000
        sats[i]["obs"]["epoch"], sats[i]["obs"]["code"] = 1000 + e, code
    return sats


def test_solver_returns_the_truth():
    """Per satellite the solver's residual differs from the truth's by: the code phase's
    rounding, 2^-33 chip = 3.4e-8 m; the receive time as a double second of week, spaced 2^-33 s
    near 5e5 s, seen through a range rate below 1 km/s, 1.2e-7 m (the solver keeps times as a whole
    second plus a fraction, so that rounding reaches the satellites' positions alone); and double
    rounding in the range itself, a few ulp of 2.6e7 m, 2e-8 m: together below 2e-7 m.  The
    position error is at most PDOP times the root of their mean square, the iteration stops at
    steps below 1e-6 m, so the bound is (2e-7 PDOP + 1e-6) m, and (2e-7 TDOP + 1e-6) / c + 2^-33 s
    for T0, with TDOP < PDOP for any sky."""
    nd = G.NavData(NAV)
    g0 = start_time()
    xyz = llh_to_ecef(*LOC)
    prns = sorted(steady_rows())
    fs = 1e6
    for t in (0, 600 * 1000, 12345678):
        for no_iono in (False, True):
            sats = exact_sats(nd, prns, g0, xyz, fs, t, no_iono)
            fix = G.pvt_solve(nd, fs, t, sats, no_iono=no_iono)
            assert fix.status == G.PVT_OK and fix.n_used == len(prns)
            err = float(np.linalg.norm(np.array(fix.xyz) - xyz))
            dt = (Fraction(fix.t0_floor) + Fraction(fix.t0_frac)) - Fraction(g0[1])
            print(t, no_iono, "error", err, "m,", float(dt), "s, pdop", fix.pdop, "rms", fix.rms,
                  "iterations", fix.iterations)
            assert 1.0 < fix.pdop < 5.0
            assert err <= 2e-7 * fix.pdop + 1e-6
            assert abs(float(dt)) <= (2e-7 * fix.pdop + 1e-6) / C_LIGHT + 2.0**-33
            assert abs(fix.t0_sec - g0[1]) <= 2.0**-33 + 2.0**-34 and fix.t0_week == g0[0]
            assert fix.rms <= 4e-7
            llh = np.array(fix.llh) * [57.2957795131, 57.2957795131, 1.0]
            assert np.allclose(llh, LOC, atol=1e-6)
    # the wrong model is seen: a file with the ionosphere, solved without
    sats = exact_sats(nd, prns, g0, xyz, fs, 0, False)
    off = G.pvt_solve(nd, fs, 0, sats, no_iono=True)
    assert off.status == G.PVT_OK and np.linalg.norm(np.array(off.xyz) - xyz) > 1.0
    nd.close()


def test_too_few_or_useless_satellites_give_a_status():
    nd = G.NavData(NAV)
    g0 = start_time()
    xyz = llh_to_ecef(*LOC)
    prns = sorted(steady_rows())
    sats = exact_sats(nd, prns, g0, xyz, 1e6, 0)
    for n in (0, 1, 3):
        fix = G.pvt_solve(nd, 1e6, 0, sats[:n])
        assert fix.status == G.PVT_FEW and fix.n_used == n
    gone = sats.copy()
    gone["obs"]["epoch"][3:] = -1                           # observables outside their jobs
    assert G.pvt_solve(nd, 1e6, 0, gone).status == G.PVT_FEW
    same = sats[[0, 0, 0, 0, 0]]                            # one direction: no geometry
    assert G.pvt_solve(nd, 1e6, 0, same).status in (G.PVT_SINGULAR, G.PVT_DIVERGED)
    assert G.pvt_solve(G.NavData(), 1e6, 0, sats).status == G.PVT_FEW    # no ephemeris at all
    assert G.pvt_solve(nd, 1e6, 0, sats[:4]).status == G.PVT_OK
    nd.close()


# ---- the physical test ---------------------------------------------------------------------
# Worst values over the fixes of each run, measured on this test (static scenario, eleven
# satellites, 12.5 s at 1 MS/s, fixes at 10 Hz from epoch 600 on; noise for 50 dB-Hz, seed 7):
#   run          distance from LOC [m]   |T0 - g0| [ns]   speed [m/s]   code against the row [chip]
MEASURED = {
    "clean16": (9.479, 15.05, 0.4639, 0.02769),
    "sc16":    (11.74, 23.90, 0.8227, 0.03531),
    "sc08":    (12.16, 24.81, 0.8109, 0.0),
    "sc01":    (13.82, 29.10, 1.1683, 0.0),
}
# The bounds are twice the worst value seen: the margin is for another noise seed's scatter, as
# trk_oracle.LEVEL and check_physical allow it.  Whatever is measured they stay under half a
# sample, c / (2 fs) = 150 m and 1 / (2 fs) = 0.5 us (one sample of code error is 300 m), and
# the code phase within half a chip of the row's.  The noise-free 9.5 m is the code loop's own
# error at one sample per chip (0.028 chip of 293 m), not the model's: the solver returns the
# truth to 1e-7 m on exact observables (above).
CAP_M, CAP_S, CAP_CHIP = C_LIGHT / (2 * 1e6), 0.5e-6, 0.5
FIRST_EPOCH, RATE_HZ = 600, 10


_tracked = {}


def tracked(fmt, clean=False):
    """exactly tests/test_track.py::tracked, computed once per input"""
    import acq_oracle as A
    if (fmt, clean) not in _tracked:
        data = O.phys_samples(fmt, clean)
        peaks, _, _ = G.acquire_host(O.phys_acq(fmt), data)
        jobs, keep = O.phys_jobs(fmt, peaks)
        assert len(jobs) == len(keep) >= 8
        rec, count = G.track_host(G.Trk(A.PHYS_FS, fmt), data, jobs, threads=8)
        _tracked[fmt, clean] = (rec, count, jobs, keep)
    return _tracked[fmt, clean]


def fix_grid(rec, count, fs, first_epoch=FIRST_EPOCH, rate=RATE_HZ):
    """(t_first, step, n_fix): multiples of fs / rate from the first at which every job is past
    first_epoch, to the last inside every job's records"""
    step = int(fs) // rate
    lo = max(int(rec["s"][j, first_epoch]) for j in range(len(count)))
    hi = min(int(rec["s"][j, count[j] - 1]) for j in range(len(count)))
    k0 = -(-lo // step)
    return k0 * step, step, (hi - 1) // step - k0 + 1


def fixes_of(nd, fs, rec, count, jobs, obs, grid, no_iono=False, week=0):
    """the fixes at the grid's instants from obs [n_job, n_fix]; every decoded subframe goes to
    the navdata first (it selects the RINEX set by IODE, or builds the set on a handle opened
    empty, which knows the week only modulo 1024: week)"""
    anchors = []
    for j, job in enumerate(jobs):
        sfs, _ = G.nav_decode(rec[j, :count[j]])
        assert len(sfs) >= 1, int(job["prn"])
        for sf in sfs:
            nd.add_subframe(int(job["prn"]), sf)
        anchors.append(sfs[0])
    t_first, step, n_fix = grid
    out = []
    for k in range(n_fix):
        sats = np.zeros(len(jobs), G.PVT_SAT_DTYPE)
        sats["obs"] = obs[:, k]
        sats["prn"] = jobs["prn"]
        sats["sf_epoch"] = [a["epoch"] for a in anchors]
        sats["sf_tow"] = [a["tow"] for a in anchors]
        out.append(G.pvt_solve(nd, fs, t_first + k * step, sats, no_iono=no_iono, week=week))
    return out


def worst_of(fixes, g0, xyz):
    """(distance [m], |T0 - g0| [s], speed [m/s]) at their worst over the fixes"""
    assert fixes and all(f.status == G.PVT_OK for f in fixes), [f.status for f in fixes]
    d = max(float(np.linalg.norm(np.array(f.xyz) - xyz)) for f in fixes)
    dt = max(abs(float(Fraction(f.t0_floor) + Fraction(f.t0_frac) - Fraction(g0[1])))
             for f in fixes)
    v = max(float(np.linalg.norm(np.array(f.vel))) for f in fixes)
    assert all(f.t0_week == g0[0] for f in fixes)
    return d, dt, v


def code_against_rows(obs, grid, jobs, keep):
    """the largest distance [chip, modulo the code period] between the observables' code phase
    and the channel rows', advanced to the same sample as check_decode does"""
    blk, nch, nav, n_per_blk = O.phys_rows()
    t_first, step, n_fix = grid
    worst = 0.0
    for j, job in enumerate(jobs):
        slot = keep[int(job["prn"])]
        for k in range(n_fix):
            b, i = divmod(t_first + k * step, n_per_blk)
            rw = blk[b][slot]
            ph = G.code_advance(rw["code0"], rw["code_step"], i, rw["icode"], rw["ibit"],
                                rw["iword"])[0]
            d = (float(obs[j, k]["code"]) / 2**32 - ph) % 1023.0
            worst = max(worst, min(d, 1023.0 - d))
    return worst


def physical(fmt, clean):
    import acq_oracle as A
    fs = A.PHYS_FS
    rec, count, jobs, keep = tracked(fmt, clean)
    grid = fix_grid(rec, count, fs)
    assert grid[2] >= 100 and grid[0] % grid[1] == 0
    obs = G.observables_host(fs, rec, count, *grid)
    assert (obs["epoch"] >= FIRST_EPOCH).all()
    nd = G.NavData(NAV)
    fixes = fixes_of(nd, float(fs), rec, count, jobs, obs, grid)
    nd.close()
    d, dt, v = worst_of(fixes, start_time(), llh_to_ecef(*LOC))
    chip = code_against_rows(obs, grid, jobs, keep) if fmt == 16 else 0.0
    return d, dt, v, chip


@pytest.mark.parametrize("run", list(MEASURED))
def test_physical_fixes(run):
    fmt, clean = {"clean16": (16, True), "sc16": (16, False), "sc08": (8, False),
                  "sc01": (1, False)}[run]
    d, dt, v, chip = physical(fmt, clean)
    print(run, "distance", d, "m, |T0 - g0|", dt * 1e9, "ns, speed", v, "m/s, code", chip, "chip")
    md, mdt, mv, mchip = MEASURED[run]
    bound = (min(2 * md, CAP_M), min(2 * mdt * 1e-9, CAP_S), 2 * mv, min(2 * mchip, CAP_CHIP))
    assert 2 * md < CAP_M and 2 * mdt * 1e-9 < CAP_S and 2 * mchip < CAP_CHIP
    assert d <= bound[0] and dt <= bound[1] and v <= bound[2]
    if fmt == 16:
        assert chip <= bound[3]


def tool_fixes(text):
    """{k: fields} of the tool's FIX lines"""
    out = {}
    for ln in text.splitlines():
        f = ln.split()
        if f and f[0] == "FIX":
            out[int(f[1])] = dict(t=float(f[3]), sats=int(f[5]), xyz=[float(v) for v in f[6:9]],
                                  llh=[float(v) for v in f[9:12]], speed=float(f[13]),
                                  week=int(f[15]), sec=float(f[16]))
    return out


def test_tool_on_the_host(tmp_path):
    """gps-sdr-pvt --host -e on the physical file prints the fixes of the physical test, from the
    first instant at which four satellites are past bit synchronisation; the --csv rows parse
    back as the motion files gps-sdr-sim -u reads do"""
    import subprocess
    import acq_oracle as A
    fs = A.PHYS_FS
    f, csv = tmp_path / "phys.bin", tmp_path / "fix.csv"
    O.phys_samples(16).tofile(f)
    rec, count, jobs, keep = tracked(16)
    grid = fix_grid(rec, count, fs)
    obs = G.observables_host(fs, rec, count, *grid)
    nd = G.NavData(NAV)
    want = fixes_of(nd, float(fs), rec, count, jobs, obs, grid)
    nd.close()
    prns = ",".join(str(p) for p in sorted(keep))
    out = subprocess.run([G.PVT_CLI_PATH, "-f", str(f), "-s", str(fs), "-b", "16", "-e", NAV,
                          f"--prn={prns}", "--host", f"--csv={csv}"], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    got = tool_fixes(out.stdout)
    k0 = grid[0] // grid[1]
    assert min(got) <= k0 and min(got) * grid[1] >= 500 * 1000
    for k, w in enumerate(want):
        g = got[k0 + k]
        assert g["sats"] == len(jobs) and g["week"] == w.t0_week
        assert np.allclose(g["xyz"], w.xyz, rtol=0, atol=0.00051), (k, g, list(w.xyz))
        assert abs(g["sec"] - w.t0_sec) < 0.6e-9 and abs(g["t"] - (k0 + k) / RATE_HZ) < 1e-9
        assert abs(g["llh"][0] - LOC[0]) < 1e-3 and abs(g["llh"][1] - LOC[1]) < 1e-3
    rows = np.loadtxt(csv, delimiter=",")
    assert rows.shape == (len(got), 4)
    for r, (k, g) in zip(rows, sorted(got.items())):
        assert abs(r[0] - g["t"]) < 0.051 and np.allclose(r[1:], g["xyz"], rtol=0, atol=0.0011)
    # the rows are a motion file: the simulator reads them back
    s = G.Scenario(NAV, motion_file=str(csv), duration=1.0, samp_freq=1e6)
    s.close()
    # no ephemeris file and 12.5 s of signal: no fix, said so, and no crash
    bare = subprocess.run([G.PVT_CLI_PATH, "-f", str(f), "-s", str(fs), f"--prn={prns}",
                           "--host", "-d", "3"], capture_output=True, text=True)
    assert bare.returncode == 0 and "FIX" not in bare.stdout and "No fix" in bare.stderr


def test_struct_sizes_match_the_c_header(tmp_path):
    """the binding's views of the new public structs have the C compiler's sizes"""
    import ctypes
    import subprocess
    from conftest import REPO
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gpssim_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d\\n", sizeof(gss_obs_t), '
                   'sizeof(gss_pvt_sat_t), sizeof(gss_pvt_fix_t), sizeof(gss_pvt_opts_t), '
                   'GSS_NAVDATA_FIELDS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", REPO + "/include", str(src), "-o", str(exe)], check=True)
    obs, sat, fix, opts, nf = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                      check=True).stdout.split())
    assert obs == G.OBS_DTYPE.itemsize == 32 and sat == G.PVT_SAT_DTYPE.itemsize == 48
    assert fix == ctypes.sizeof(G.PvtFix) == 136 and opts == ctypes.sizeof(G._PvtOpts)
    assert nf == len(G.NAVDATA_FIELDS)
