"""The time of gss_dev_open (events, streams and the constant tables it uploads) for the library
GSS_LIB_PATH names (else the in-tree build): after one open that pays for the runtime's start,
N opens timed with the host clock, each closed again before the next (profiles/refactor_handle/).
The open returns after its synchronous copies, so the clock covers them.

usage: [GSS_LIB_PATH=... GSS_ALLOW_LIB_OVERRIDE=1] python tools/dev_open_time.py TAG [N]"""
import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import gpssim_amd as G
tag = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 25
G.Device(0).close()
times = []
for _ in range(n):
    t0 = time.perf_counter()
    d = G.Device(0)
    times.append((time.perf_counter() - t0) * 1e3)
    d.close()
t = sorted(times)
print(f"{tag:8} gss_dev_open: median {t[len(t) // 2]:.3f} ms min {t[0]:.3f} max {t[-1]:.3f} "
      f"({n} opens)", flush=True)
