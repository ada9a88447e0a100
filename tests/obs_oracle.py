"""The observables of tracked signals (include/gpssim_amd.h, gss_obs_t) restated
in Python integers, and the inputs the CPU and GPU tests share.

The restatement goes by the definition, instant by instant: it finds the epoch an instant lies
in and evaluates the two lines there, whereas the library walks the records and lets each write
the instants it owns."""
from bisect import bisect_right

import numpy as np

import gpssim_amd as G
import trk_oracle as O

M = O.M

# csrc/hip/gss_obs.hip: records a lane, a row of 16 lanes, a wave and a workgroup take per tile
LANE = 4
ROW = 16 * LANE
WAVE = 64 * LANE
TILE = 256 * LANE
# the counts of the edge family: every unit of the scan minus one, exact and plus one, two tiles
# plus one, and the counts 0, 1, 2 the definition treats apart
EDGE_COUNTS = (0, 1, 2, LANE - 1, LANE, LANE + 1, ROW - 1, ROW, ROW + 1, WAVE - 1, WAVE, WAVE + 1,
               TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
BIG = 70000                       # one long job beside many of three records
BIG_JOBS = 300                    # more jobs than the 256 CUs


def s64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def observables(fs, rec, count, t_first, step, n_fix):
    """OBS_DTYPE [n_job, n_fix] by the definition"""
    cs_nom = O.cs_nominal(fs)
    out = np.zeros((len(count), n_fix), G.OBS_DTYPE)
    out["epoch"] = -1
    for j, c in enumerate(int(x) for x in count):
        if c < 1:
            continue
        s = [int(x) for x in rec["s"][j, :c]]
        w = [int(x) for x in rec["w"][j, :c]]
        cs = [cs_nom + int(x) for x in rec["dcs"][j, :c]]
        phi, A = [0], [0]
        for e in range(c - 1):
            n = s[e + 1] - s[e]
            phi.append(phi[e] + n * cs[e] - M)
            A.append(A[e] + n * w[e])
        last = phi[-1] % (1 << 64)
        n_last = -(-(M - last) // cs[-1]) if cs[-1] > 0 and last < M else 0
        ends = s[1:] + [s[-1] + n_last]
        o = out[j]
        for k in range(n_fix):
            t = t_first + k * step
            e = bisect_right(s, t) - 1
            if e < 0 or t >= ends[e]:
                continue
            o[k] = (s64(phi[e] + (t - s[e]) * cs[e]), s64(A[e] + (t - s[e]) * w[e]), e, w[e], 0)
    return out


def synthetic(fs, counts, seed, pitch=None, s0=None):
    """(rec [n_job, pitch], count): records whose s, w and dcs alone are set; the lengths are
    those the code phase implies, w is any int32, dcs within +-3000"""
    rng = np.random.default_rng(seed)
    cs_nom = O.cs_nominal(fs)
    pitch = max(max(counts), 1) if pitch is None else pitch
    rec = np.zeros((len(counts), pitch), G.TRK_REC_DTYPE)
    for j, c in enumerate(counts):
        w = rng.integers(-2**31, 2**31, size=c, dtype=np.int64)
        dcs = rng.integers(-3000, 3001, size=c, dtype=np.int64)
        s, phi = (int(rng.integers(0, 50)) if s0 is None else s0[j]), 0
        for e in range(c):
            rec[j, e]["s"], rec[j, e]["w"], rec[j, e]["dcs"] = s, w[e], dcs[e]
            cs = cs_nom + int(dcs[e])
            n = -(-(M - phi) // cs)
            s += n
            phi += n * cs - M
    return rec, np.array(counts, np.int32)


def span(rec, count):
    """(first sample of any job, one past the last record's first sample of any job)"""
    lo = min(int(rec["s"][j, 0]) for j, c in enumerate(count) if c > 0)
    hi = max(int(rec["s"][j, c - 1]) for j, c in enumerate(count) if c > 0)
    return lo, hi


_cases = {}


def case(name):
    """name -> dict(fs, rec, count, grids): grids is a list of (t_first, step, n_fix)"""
    if name in _cases:
        return _cases[name]
    if name == "edges":
        # 4 kS/s: epochs of 3 and 4 samples; with step 3 every epoch of every job holds an instant
        fs = 4000
        rec, count = synthetic(fs, EDGE_COUNTS, 11, pitch=2 * TILE + 4)
        lo, hi = span(rec, count)
        grids = [(lo - 7, 3, (hi - lo) // 3 + 12), (lo - 2, 1, 300), (lo + 5, 10 * (hi - lo), 3)]
    elif name == "small":
        # counts 0, 1, 2 and more at 1 MS/s, pitch > count; instants before s_0, at s_e, at
        # s_e + n_e - 1, at the end of the last epoch and beyond it, step 1 across a boundary
        fs = 1000000
        rec, count = synthetic(fs, (0, 1, 2, 7), 5, pitch=9, s0=(0, 40, 40, 40))
        s1 = int(rec["s"][3, 1])
        grids = [(38, 1, 8), (s1 - 3, 1, 6), (40, 1, 7100), (40, 500, 20), (-5, 10**7, 2),
                 (0, 1, 0)]
    elif name == "big":
        fs = 4000
        rec, count = synthetic(fs, (3,) * 150 + (BIG,) + (3,) * (BIG_JOBS - 151), 3)
        lo, hi = span(rec, count)
        grids = [(lo - 1, (hi - lo) // 400 + 1, 420)]
    elif name == "jumps":
        # records 2^40 samples apart at the ends of w: the accumulated carrier wraps modulo 2^64
        fs = 1000000
        rec = np.zeros((2, 40), G.TRK_REC_DTYPE)
        for j, w in enumerate((-2**31, 2**31 - 1)):
            rec["s"][j] = 5 + (np.arange(40, dtype=np.int64) << 40)
            rec["w"][j] = w
            rec["dcs"][j] = -((np.arange(40) * 37) % 11)
        count = np.array([40, 33], np.int32)
        grids = [(0, 1 << 39, 90)]
    else:
        c = O.case(name)                          # the tracking oracle's own records
        fs, rec, count = c["fs"], c["rec"], np.asarray(c["count"], np.int32)
        lo, hi = span(rec, count)
        T = -(-fs // 1000)
        grids = [(lo - 3, T // 3 + 1, 3 * (hi - lo + 2 * T) // T + 12), (lo - 1, 1, 2 * T + 5)]
    _cases[name] = dict(fs=fs, rec=rec, count=count, grids=grids)
    return _cases[name]


TRACKED = O.FEEDBACK + O.ENDS
NAMES = ["small", "edges", "big", "jumps"] + TRACKED
_want = {}


def want(name, g):
    """the oracle's observables of grid g of a case, computed once"""
    if (name, g) not in _want:
        c = case(name)
        _want[name, g] = observables(c["fs"], c["rec"], c["count"], *c["grids"][g])
    return _want[name, g]


def same(obs, wobs):
    assert obs.shape == wobs.shape
    if not np.array_equal(obs.view(np.uint8), wobs.view(np.uint8)):
        for f in ("epoch", "w", "code", "adr", "pad"):
            bad = np.argwhere(obs[f] != wobs[f])
            assert not len(bad), (f, bad[:5], [(obs[f][tuple(b)], wobs[f][tuple(b)])
                                               for b in bad[:5]])
