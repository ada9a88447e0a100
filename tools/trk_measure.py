#!/usr/bin/env python3
"""Timing of the tracking kernel (gss_track_device).

    tools/trk_measure.py                      every shape: fast and plain form in alternating
                                              child processes, then the host on 16 threads
    tools/trk_measure.py --one SHAPE PATH     one process: a warm-up call, then the median of
                                              --reps calls between device events; one JSON line

Shapes (random SC16 samples: the loops never lock, the work per epoch is the same):
    default   2.6 MS/s, 12 jobs x 30,000 epochs       the tool's default shape
    split     2.6 MS/s, 360 jobs x 1,000 epochs       --split=1: 12 PRNs x 30 windows of the file
    wide      20 MS/s, 8 jobs x 2,000 epochs
Logs go to profiles/track/ (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))

SHAPES = {"default": (2600000, 12, 30000, 1), "split": (2600000, 12, 1000, 30),
          "wide": (20000000, 8, 2000, 1)}


def make_jobs(G, fs, n_prn, ne, n_win):
    import numpy as np
    T = fs // 1000
    jobs = np.zeros(n_prn * n_win, G.TRK_JOB_DTYPE)
    for w in range(n_win):
        for p in range(n_prn):
            hz = -4000 + 700 * p
            jobs[w * n_prn + p] = (w * (ne + 2) * T + 37 * p, 1 + (5 * p) % 32,
                                   (hz * 2**32 + fs // 2) // fs, ne, 0)
    return jobs, (n_win * (ne + 2) + 2) * T


def one(shape, path, reps, host):
    import numpy as np
    import torch
    import gpssim_amd as G
    fs, n_prn, ne, n_win = SHAPES[shape]
    jobs, N = make_jobs(G, fs, n_prn, ne, n_win)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randint(-2000, 2000, (2 * N,), dtype=torch.int16, device="cuda", generator=g)
    trk = G.Trk(fs, 16)
    out = {"shape": shape, "fs": fs, "jobs": len(jobs), "epochs": ne, "path": path}
    if host:
        xh = x.cpu().numpy()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            rec, count = G.track_host(trk, xh, jobs, n=N, threads=16)
            t.append(time.perf_counter() - t0)
        ms = 1e3 * sorted(t)[1]
        out["path"] = "host16"
    else:
        if path == "plain":
            os.environ["GSS_TRK_PATH"] = "plain"
        dev = G.Device(0)
        rec = torch.zeros(len(jobs) * ne * 64, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(len(jobs), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        t = []
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dev.track(trk, x.data_ptr(), N, jobs, rec.data_ptr(), ne, cnt.data_ptr(), stream=st)
            b.record()
            torch.cuda.synchronize()
            if r:
                t.append(a.elapsed_time(b))
        ms = sorted(t)[len(t) // 2]
        count = cnt.cpu().numpy()
        out["all_ms"] = [round(v, 3) for v in t]
        dev.close()
    assert (count == ne).all(), count
    total = int(count.sum())
    out.update(ms=round(ms, 3), us_per_epoch_job=round(1e3 * ms / total, 4),
               signal_s_per_s=round(total * 1e-3 / (ms * 1e-3), 1))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("SHAPE", "PATH"))
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="default,split,wide")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track"))
    a = ap.parse_args()
    if a.one:
        one(a.one[0], a.one[1], a.reps, a.host)
        return
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "trk_measure.jsonl"), "w") as log:
        for shape in a.shapes.split(","):
            runs = [("fast", False), ("plain", False), ("fast", False), ("plain", False),
                    ("fast", True)]
            for path, host in runs:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, path,
                       "--reps", str(a.reps)] + (["--host"] if host else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
                if r.returncode != 0:          # a failed child ends the measurement: no retries
                    sys.stderr.write(r.stdout + r.stderr)
                    sys.exit(r.returncode or 1)
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()


if __name__ == "__main__":
    main()
