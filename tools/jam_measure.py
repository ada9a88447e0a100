"""Measurements of the jammers (logs in profiles/jam/): the jam kernel's time per
headline window (2,999 blocks x 260,000 samples) with 0, 1 and 4 jammers, with and without noise,
at each format, beside the unchanged impair kernel in the same process, alternating; and the wall
time of the 300 s -b 16 CLI run with --jam=cw,30,0 against the same command without it and
against another build's gps-sdr-sim (GSS_PARENT_CLI, e.g. the parent commit's), interleaved with
a rotating order.

usage: python tools/jam_measure.py [--cli-only | --kernels-only] [--rounds=N]"""
import os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import numpy as np
import gpssim_amd as G

NAV = os.path.join(REPO, "tests", "golden", "data", "brdc3540.14n")
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
    work = torch.empty_like(iq)
    out = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    sigma = int(np.floor(256 * 250 * np.sqrt(2.6e6 / (2 * 10 ** 4.5)) + 0.5))
    st = torch.cuda.current_stream().cuda_stream
    fs = 2.6e6
    pool = [G.jam_make(fs, 30.0, 0.0), G.jam_make(fs, 10.0, -1.0e6, 1.0e6, 137e-6),
            G.jam_make(fs, 20.0, 137e3, 0.0, 0.0, 1e-3, 0.1),
            G.jam_make(fs, 0.0, 1.0e6, -1.0e6, 1e-3, 2e-3, 0.5)]

    def once(fmt, imp, jam):
        """one launch over the window, device events; jam None: the impair kernel"""
        if fmt == 16:
            work.copy_(iq)
        src = work.data_ptr() if fmt == 16 else iq.data_ptr()
        dst = work.data_ptr() if fmt == 16 else out.data_ptr()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if jam is None:
            dev.impair_device(imp, src, 1, N, fmt, dst, stream=st)
        else:
            dev.jam_device(imp, jam, src, 1, N, fmt, dst, stream=st)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for fmt, bytes_out in ((16, 4), (8, 2), (1, 0.25)):
        legs = [("impair kernel, noise", G.Impair(sigma, 0, 7), None)]
        for nj in (0, 1, 4):
            legs.append((f"jam kernel, noise, {nj} jammers", G.Impair(sigma, 0, 7), pool[:nj]))
        legs.append(("impair kernel, sigma 0", G.Impair(0, 0, 7), None))
        for nj in (0, 1, 4):
            legs.append((f"jam kernel, no noise, {nj} jammers", G.Impair(0, 0, 7), pool[:nj]))
        times = {name: [] for name, _, _ in legs}
        for rep in range(REPS + 1):                           # the first round warms up
            for name, imp, jam in legs[rep % len(legs):] + legs[:rep % len(legs)]:
                t = once(fmt, imp, jam)
                if rep:
                    times[name].append(t)
        traffic = N * (4 + bytes_out)
        base = median(times["impair kernel, noise"])
        for name, _, _ in legs:
            t = times[name]
            med = median(t)
            print(f"-b {fmt:<2} {name:34}: median {med:.3f} ms (min {min(t):.3f}, max {max(t):.3f}) "
                  f"= {med / base:.2f} x the impair kernel; {med / N * 1e9:.2f} ps per sample; "
                  f"{traffic / med / 1e9:.3f} TB/s of the traffic n (4 + bytes out)", flush=True)
    dev.close()


def cli():
    new = G.CLI_PATH
    old = os.environ.get("GSS_PARENT_CLI")
    common = ["-e", NAV, "-l", "30.286502,120.032669,100", "-o", "/dev/null", "-d", "300", "-b",
              "16"]
    legs = [("parent plain", old, []), ("new plain", new, []),
            ("new --jam=cw,30,0", new, ["--jam=cw,30,0"])]
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
            print(f"cli 300 s -b 16 {tag:18}: " + " ".join(f"{x:.3f}" for x in v) +
                  f"  (first dropped) median {median(v[1:]):.3f} s", flush=True)


if "--cli-only" not in sys.argv:
    kernels()
if "--kernels-only" not in sys.argv:
    cli()
