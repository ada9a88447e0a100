"""Measurements of the multipath echoes (logs in profiles/echo/): the echo kernel's
time per headline window (2,999 blocks x 260,000 samples, the rows of the 300 s scenario) with one
echo on one satellite and one echo on every satellite, in its carried and its plain form, beside
the unchanged impair kernel and the render (the exact path's gss_synth_device over the first
blocks of the window, scaled) in the same process, device events, median of 5 after a warm-up
with the order rotating; and the wall time of the 300 s -b 16 CLI run with --multipath=all,150,6
against the same command without it and against another build's gps-sdr-sim (GSS_PARENT_CLI,
e.g. the parent commit's), interleaved with a rotating order.

usage: python tools/echo_measure.py [--cli-only | --kernels-only] [--rounds=N]"""
import os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import numpy as np
import gpssim_amd as G

NAV = os.path.join(REPO, "tests", "golden", "data", "brdc3540.14n")
LOC = (30.286502, 120.032669, 100.0)
NBLK, NPB = 2999, 260000
N = NBLK * NPB
RENDER_BLKS = 64                       # blocks the render yardstick renders (scaled to the window)
ROUNDS = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--rounds=")), 7)
REPS = 5


def median(v):
    w = sorted(v)
    return (w[(len(w) - 1) // 2] + w[len(w) // 2]) / 2


def kernels():
    import torch
    dev = G.Device(0)
    print("build:", G.lib().gss_build_info().decode(), flush=True)
    scn = G.Scenario(NAV, llh=LOC, duration=300.0, samp_freq=2.6e6, data_format=16)
    blk, nch, ck = scn.all_blocks(with_ck=True)
    nav = scn.nav_table()
    assert len(nch) == NBLK and scn.n_per_blk == NPB
    scn.close()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_blk, d_nch, d_ck, d_ca, d_nav = up(blk), up(nch), up(ck), up(G.ca_table()), up(nav)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    iq = torch.randint(-1400, 1401, (2 * N,), dtype=torch.int16, device="cuda", generator=g)
    st = torch.cuda.current_stream().cuda_stream
    prn = int(blk[0, 0]["ca_tbl"]) + 1
    print(f"channels per block: {nch.min()}..{nch.max()}, the single satellite: PRN {prn}", flush=True)
    dev.reserve(RENDER_BLKS, NPB)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def echo(es, plain):
        def run():
            if plain:
                os.environ["GSS_ECHO_PATH"] = "plain"
            else:
                os.environ.pop("GSS_ECHO_PATH", None)
            t = timed(lambda: dev.echo_device(es, d_blk.data_ptr(), d_nch.data_ptr(), NBLK, NPB,
                                              d_ca.data_ptr(), 32, d_nav.data_ptr(), len(nav), 1,
                                              iq.data_ptr(), stream=st))
            os.environ.pop("GSS_ECHO_PATH", None)
            return t
        return run

    def impair():
        return timed(lambda: dev.impair_device(G.Impair(0, 0, 7), iq.data_ptr(), 1, N, 16,
                                               iq.data_ptr(), stream=st))

    def render():
        t = timed(lambda: dev.synth_device(d_blk.data_ptr(), d_nch.data_ptr(), int(nch.max()),
                                           d_ca.data_ptr(), 32, d_nav.data_ptr(), len(nav),
                                           RENDER_BLKS, NPB, 16, iq.data_ptr(), stream=st,
                                           ck_ptr=d_ck.data_ptr()))
        return t * NBLK / RENDER_BLKS

    one = [G.echo_make(2.6e6, prn, 150.0, 6.0)]
    every = [G.echo_make(2.6e6, 0, 150.0, 6.0)]
    legs = [("impair kernel, sigma 0", impair), (f"render, exact path ({RENDER_BLKS} blocks, scaled)", render),
            ("echo kernel, one satellite, carried", echo(one, False)),
            ("echo kernel, one satellite, plain", echo(one, True)),
            ("echo kernel, every satellite, carried", echo(every, False)),
            ("echo kernel, every satellite, plain", echo(every, True))]
    times = {name: [] for name, _ in legs}
    for rep in range(REPS + 1):                               # the first round warms up
        for name, f in legs[rep % len(legs):] + legs[:rep % len(legs)]:
            t = f()
            if rep:
                times[name].append(t)
    base = median(times["impair kernel, sigma 0"])
    for name, _ in legs:
        t = times[name]
        med = median(t)
        print(f"{name:44}: median {med:.3f} ms (min {min(t):.3f}, max {max(t):.3f}) = "
              f"{med / base:.2f} x the impair kernel; {med / N * 1e9:.2f} ps per sample", flush=True)
    dev.close()


def cli():
    new = G.CLI_PATH
    old = os.environ.get("GSS_PARENT_CLI")
    common = ["-e", NAV, "-l", "%.6f,%.6f,%g" % LOC, "-o", "/dev/null", "-d", "300", "-b", "16"]
    legs = [("parent plain", old, []), ("new plain", new, []),
            ("new --multipath=all,150,6", new, ["--multipath=all,150,6"])]
    res = {tag: [] for tag, _, _ in legs}
    for rep in range(ROUNDS):
        for tag, exe, more in legs[rep % 3:] + legs[:rep % 3]:    # the order rotates
            if exe is None:
                continue
            t0 = time.perf_counter()
            p = subprocess.run([exe] + common + more, capture_output=True, text=True, timeout=400)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                print(tag, "FAILED", p.stderr[-500:], flush=True)
                sys.exit(1)
            res[tag].append(dt)
    for tag, v in res.items():
        if v:
            print(f"cli 300 s -b 16 {tag:26}: " + " ".join(f"{x:.3f}" for x in v) +
                  f"  (first dropped) median {median(v[1:]):.3f} s", flush=True)


if "--cli-only" not in sys.argv:
    kernels()
if "--kernels-only" not in sys.argv:
    cli()
