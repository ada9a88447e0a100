"""Measurements of the additive noise (logs in profiles/impair/): the render
kernel's time per headline window (gss_dev_timing_lin), the impair kernel's time per window and
its share of the HBM roofline at each format, and the wall time of the 300 s -b 16 and 24 h -b 1
CLI runs with --cn0=45 against the same commands without it, interleaved (GSS_PARENT_CLI: the
gps-sdr-sim of another build, e.g. the parent commit's, run beside them).

usage: python tools/impair_measure.py [--cli-only | --kernels-only]"""
import os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import numpy as np
import torch
import gpssim_amd as G

NAV = os.path.join(REPO, "tests", "golden", "data", "brdc3540.14n")
LOC = (30.286502, 120.032669, 100.0)
NBLK, NPB = 2999, 260000
CLI_ONLY = "--cli-only" in sys.argv
ROUNDS = 7
N = NBLK * NPB


def kernels():
    dev = G.Device(0)
    print("build:", G.lib().gss_build_info().decode(), flush=True)

    # (1) the render kernel of the headline window, gss_dev_timing_lin, this process
    s = G.Scenario(NAV, llh=LOC, duration=300.0, data_format=16)
    tot = [0]
    def sink(buf, first, nb): tot[0] += len(buf)
    dev.run(s, sink, batch=128, threads=16)          # warm
    s.close()
    for rep in range(2):
        s = G.Scenario(NAV, llh=LOC, duration=300.0, data_format=16)
        dev.timing_reset()
        t0 = time.perf_counter()
        dev.run(s, sink, batch=128, threads=16)
        wall = time.perf_counter() - t0
        n, ms = dev.timing_lin()
        print(f"render -b 16 window: {n} fast-path launches (ring of the last 256 at most), avg {ms:.4f} ms "
              f"-> {ms * 24:.3f} ms per 2,999-block window at 24 launches of 128 blocks "
              f"(last is 55 blocks); run wall {wall:.3f} s", flush=True)
        s.close()

    # (2) the impair kernel over one headline window of SC16 samples
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    iq = torch.randint(-1400, 1401, (2 * N,), dtype=torch.int16, device="cuda", generator=g)
    work = torch.empty_like(iq)
    out = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    imp = G.Impair(int(np.floor(256 * 250 * np.sqrt(2.6e6 / (2 * 10 ** 4.5)) + 0.5)), 0, 7)
    st = torch.cuda.current_stream().cuda_stream
    for fmt, bytes_out in ((16, 4), (8, 2), (1, 0.25)):
        for s0, tag in ((0, "even start"), (1, "odd start")):
            times = []
            for rep in range(6):
                if fmt == 16:
                    work.copy_(iq)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dev.impair_device(imp, work.data_ptr() if fmt == 16 else iq.data_ptr(), s0, N, fmt,
                                  work.data_ptr() if fmt == 16 else out.data_ptr(), stream=st)
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b))
            t = sorted(times[1:])
            med = t[len(t) // 2]
            traffic = N * (4 + bytes_out)
            print(f"impair -b {fmt:<2} {tag:10}: median {med:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}; first "
                  f"{times[0]:.3f}) per window of {N} samples = {N / med / 1e6:.1f} GS/s; traffic "
                  f"{traffic / 1e9:.3f} GB -> {traffic / med / 1e9:.3f} TB/s = "
                  f"{traffic / med / 1e9 / 6.29:.3f} of 6.29 TB/s measured copy rate, "
                  f"{traffic / med / 1e9 / 8.0:.3f} of 8 TB/s spec", flush=True)
    dev.close()
    del iq, work, out
    torch.cuda.empty_cache()



if not CLI_ONLY:
    kernels()
if "--kernels-only" in sys.argv:
    sys.exit(0)

# (3) CLI wall times, parent build (plain) and this build (plain, --cn0=45), interleaved
new = G.CLI_PATH
old = os.environ.get("GSS_PARENT_CLI")
common = ["-e", NAV, "-l", "30.286502,120.032669,100", "-o", "/dev/null"]
runs = {"300 s -b 16": ["-d", "300", "-b", "16"], "24 h -b 1": ["-d", "86400", "-b", "1"]}
for name, extra in runs.items():
    res = {"parent plain": [], "new plain": [], "new --cn0=45": []}
    legs = [("parent plain", old, []), ("new plain", new, []),
            ("new --cn0=45", new, ["--cn0=45", "--seed=7"])]
    for rep in range(ROUNDS):
        for tag, exe, more in legs[rep % 3:] + legs[:rep % 3]:    # the order rotates
            if exe is None:
                continue
            t0 = time.perf_counter()
            p = subprocess.run([exe] + common + extra + more, capture_output=True, text=True,
                               timeout=400)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                print(tag, "FAILED", p.stderr[-500:], flush=True)
                sys.exit(1)
            res[tag].append(dt)
    for tag, v in res.items():
        if not v:
            continue
        w = sorted(v[1:])
        print(f"cli {name:12} {tag:14}: " + " ".join(f"{x:.3f}" for x in v) +
              f"  (first dropped) median {(w[(len(w) - 1) // 2] + w[len(w) // 2]) / 2:.3f} s",
              flush=True)
