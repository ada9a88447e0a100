"""Host time of the carrier chains (csrc/host/carr_chain.c) for the library GSS_LIB_PATH names
(else the in-tree build): one batch of 2,048 blocks at 2.6 MS/s (static, 12 channels: the batch
of the planner-bound runs), its walks, records and links made once; then the median of REPS
timed calls, at 1 and at 8 threads, of
  carr_chain (no checkpoints), carr_chain_spec, carr_chain_records, spec_links + carr_chain_linked.
Run parent and head in alternating processes (profiles/refactor_chain/).

usage: [GSS_LIB_PATH=... GSS_ALLOW_LIB_OVERRIDE=1] python tools/chain_time.py TAG [REPS]"""
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import gpssim_amd as G

tag = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
NAV = os.path.join(REPO, "tests", "golden", "data", "brdc3540.14n")
NB = 2048

# a receiver that sees twelve satellites through all of these blocks
s = G.Scenario(NAV, llh=(55.75, 37.6, 100.0), duration=300.0, samp_freq=2.6e6)
n = s.n_per_blk
b0, n0, c0 = s.next_deferred(100, threads=8)             # past the slots' first rows (restarts)
carr, _ = G.carr_chain(s.carrier(), b0, n0, c0, n, with_ck=False)
blk, nch, chain = s.next_deferred(NB, threads=8)
assert len(nch) == NB and set(nch.tolist()) == {12}
gi = G.carr_chain_guess(carr, blk, nch, chain, n)
spec = G.spec_host(gi, n, threads=8).reshape(gi.shape)
rec = G.spec_records(gi, spec, n, threads=8)
link = np.zeros((NB, G.MAXCH), G.SPEC_LINK_DTYPE)
L, p = G.lib(), G._ptr
hit = C.c_int(0)


# the C calls themselves, on preallocated arrays: the binding's copies are not the subject
def exact(c, t):
    return L.gss_carr_chain(p(c), p(blk), p(nch), p(chain), NB, n, 0, None, t)


def spec_chain(c, t):
    return L.gss_carr_chain_spec(p(c), p(blk), p(nch), p(chain), NB, n, p(gi), p(spec), t,
                                 C.byref(hit))


def records(c, t):
    return L.gss_carr_chain_records(p(c), p(blk), p(nch), p(chain), NB, n, p(rec), t,
                                    C.byref(hit))


def linked(c, t):
    rc = L.gss_spec_links(p(nch), p(chain), NB, n, p(gi), p(spec), p(link), t)
    return rc or L.gss_carr_chain_linked(p(c), p(blk), p(nch), p(chain), NB, n, p(gi), p(spec),
                                         p(link), t, C.byref(hit))


print(f"{tag:8} rows {int(nch.sum())} channels {sorted(set(nch.tolist()))} reps {reps}",
      flush=True)
for name, fn in (("carr_chain", exact), ("carr_chain_spec", spec_chain),
                 ("carr_chain_records", records), ("links+chain_linked", linked)):
    for threads in (1, 8):
        times = []
        for _ in range(reps + 2):
            c = carr.copy()
            t0 = time.perf_counter()
            rc = fn(c, threads)
            times.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        t = sorted(times[2:])                            # two calls to warm the pool and caches
        print(f"{tag:8} {name:20} t{threads} median {t[len(t) // 2]:8.3f} ms  min {t[0]:8.3f}  "
              f"max {t[-1]:8.3f}  hits {hit.value if fn is not exact else '-'}", flush=True)
