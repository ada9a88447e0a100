"""Measurements of the front-end filter (logs in profiles/fir/): the filter kernel's
time per headline window (2,999 blocks x 260,000 samples) with 15, 31 and 63 taps for the three
output formats, in its staged and its plain form, beside the unchanged impair kernel in the same
process, device events, median of 5 after a warm-up with the order rotating; and the wall time of
the 300 s -b 16 CLI run with --bandwidth=2000000 against the same command without it and against
another build's gps-sdr-sim (GSS_PARENT_CLI, e.g. the parent commit's), interleaved with a
rotating order.

usage: python tools/fir_measure.py [--cli-only | --kernels-only] [--rounds=N] [--no-plain]"""
import os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import gpssim_amd as G

NAV = os.path.join(REPO, "tests", "golden", "data", "brdc3540.14n")
LOC = (30.286502, 120.032669, 100.0)
NBLK, NPB = 2999, 260000
N = NBLK * NPB
ROUNDS = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--rounds=")), 7)
REPS = 5


def median(v):
    w = sorted(v)
    return (w[(len(w) - 1) // 2] + w[len(w) // 2]) / 2


def kernels():
    import torch
    dev = G.Device(0)
    print("build:", G.lib().gss_build_info().decode(), flush=True)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    iq = torch.randint(-1400, 1401, (2 * N,), dtype=torch.int16, device="cuda", generator=g)
    out = torch.empty(4 * N, dtype=torch.uint8, device="cuda")
    halo = torch.randint(-1400, 1401, (2 * 63,), dtype=torch.int16, device="cuda", generator=g)
    st = torch.cuda.current_stream().cuda_stream

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def fir(taps, fmt, plain):
        f = G.fir_make(2.6e6, 2.0e6, taps)

        def run():
            if plain:
                os.environ["GSS_FIR_PATH"] = "plain"
            else:
                os.environ.pop("GSS_FIR_PATH", None)
            t = timed(lambda: dev.fir_device(f, iq.data_ptr(), halo.data_ptr(), N, fmt,
                                             out.data_ptr(), stream=st))
            os.environ.pop("GSS_FIR_PATH", None)
            return t
        return run

    def impair(fmt):
        return lambda: timed(lambda: dev.impair_device(G.Impair(0, 0, 7), iq.data_ptr(), 1, N, fmt,
                                                       out.data_ptr(), stream=st))

    legs = [(f"impair kernel, sigma 0, -b {fmt}", impair(fmt)) for fmt in (16, 8, 1)]
    for fmt in (16, 8, 1):
        for taps in (15, 31, 63):
            legs.append((f"filter, {taps} taps, -b {fmt}, staged", fir(taps, fmt, False)))
            if "--no-plain" not in sys.argv:
                legs.append((f"filter, {taps} taps, -b {fmt}, plain", fir(taps, fmt, True)))
    times = {name: [] for name, _ in legs}
    for rep in range(REPS + 1):                               # the first round warms up
        for name, f in legs[rep % len(legs):] + legs[:rep % len(legs)]:
            t = f()
            if rep:
                times[name].append(t)
    base = median(times["impair kernel, sigma 0, -b 16"])
    for name, _ in legs:
        t = times[name]
        med = median(t)
        print(f"{name:40}: median {med:.3f} ms (min {min(t):.3f}, max {max(t):.3f}) = "
              f"{med / base:.2f} x the impair kernel (-b 16); {med / N * 1e9:.2f} ps per sample",
              flush=True)
    dev.close()


def cli():
    new = G.CLI_PATH
    old = os.environ.get("GSS_PARENT_CLI")
    common = ["-e", NAV, "-l", "%.6f,%.6f,%g" % LOC, "-o", "/dev/null", "-d", "300", "-b", "16"]
    legs = [("parent plain", old, []), ("new plain", new, []),
            ("new --bandwidth=2000000", new, ["--bandwidth=2000000"])]
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
