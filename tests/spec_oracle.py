"""Synthetic rows for the run-ahead carrier walks (gss_spec_host on the CPU; gss_spec_kernel, the
row-shared cycle cache of sc_seg_walk and gss_spec_rec_kernel on the GPU) and the property their
results must have, stated with the brute-force carrier loop alone (oracle.carr_brute, the
reference's step restated in oracle/synth_oracle.c): nothing here reads gss_phase.h.  Shared by
tests/test_spec_walk.py, tests/test_gpu_spec_walk.py and tests/test_gpu_parity.py.

A walk (gpssim_amd.SPEC_DTYPE) of a row (SPEC_IN_DTYPE: start g, step s, k segments starting at
samples P[j] from values W[j]) claims, per segment: the value `end` at the segment's last sample,
whether that last step wrapped, and an interval [dlo, dhi] such that a start moved by any
multiple d of the post-wrap lattice unit inside it moves the end by exactly d.  A claim that is
too wide lets the chain translate a block it should have walked, so every claim is checked at
both ends of its interval."""
import math

import numpy as np

import gpssim_amd as G
import oracle

TOP = 1.0 - 2.0 ** -53                       # the largest carrier phase
FAMILIES = 7

# Power-of-two steps from starts on their lattice: every value is a multiple of the step and
# lands exactly on binade ends.  The walkers' margins once left the walked start itself out of a
# non-empty interval there ([2^-53, ...] ascending, [..., -2^-53] descending); such a segment
# now reports no interval (gss_spec_seg_walk).
LATTICE_ROWS = [(0.0, 2.0 ** -11), (TOP, 2.0 ** -16), (TOP, -2.0 ** -8), (0.0, 2.0 ** -4),
                (TOP, -2.0 ** -11), (0.0, -2.0 ** -6)]


def _step(rng, fam):
    """one step (cycles per sample) of family fam"""
    sign = 1.0 if rng.random() < 0.5 else -1.0
    if fam == 0:                             # +-60 Hz at 2.6 MS/s, crowded towards zero Doppler
        return rng.uniform(-1.0, 1.0) ** 3 * 60.0 / 2.6e6
    if fam == 1:                             # +-6 kHz at 2.6 MS/s
        return rng.uniform(-6e3, 6e3) / 2.6e6
    if fam == 2:                             # +-6 kHz at 20 MS/s: cycles ten times longer
        return rng.uniform(-6e3, 6e3) / 2.0e7
    if fam == 3:                             # +-40 kHz at 1 MS/s: LEO-sized Doppler
        return rng.uniform(-4e4, 4e4) / 1.0e6
    if fam == 4:                             # powers of two
        return sign * 2.0 ** -int(rng.integers(3, 21))
    if fam == 5:                             # 1/s within 1e-12 of an integer
        return sign * (1.0 / int(rng.integers(5, 3001)) + (1e-12 if rng.random() < 0.5 else -1e-12))
    return rng.uniform(-0.45, 0.45)


def rows(seed, count):
    """count (g, s) pairs, the same for the same seed: the step families in turn (shifted by one
    every FAMILIES rows, so that the overrides below meet every family), every 7th step moved to a
    round-half-even tie (m + 0.5) 2^-53, every 11th start 0 and every 13th 1 - 2^-53"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        s = _step(rng, (i + i // FAMILIES) % FAMILIES)
        g = float(rng.random())
        if i % 7 == 6:
            u = 2.0 ** -53
            s = math.copysign((math.floor(abs(s) / u) + 0.5) * u, s)
        if i % 11 == 10:
            g = 0.0
        if i % 13 == 12:
            g = TOP
        assert s != 0.0 and abs(s) < 0.5 and 0.0 <= g < 1.0
        out.append((g, float(s)))
    return out


def spec_in(rows, k0=True):
    """the rows as SPEC_IN_DTYPE: k = 0 (the walker guesses the segment starts; k0 = False: one
    segment, no guesses), pad = -1 (no previous row)"""
    gi = np.zeros(len(rows), G.SPEC_IN_DTYPE)
    gi["g"] = [r[0] for r in rows]
    gi["s"] = [r[1] for r in rows]
    gi["k"] = 0 if k0 else 1
    gi["pad"] = -1
    return gi


def _wrapped(x, s, at):
    """step `at` (>= 1) of the brute-force chain from x is a wrap: the value falls (s > 0) or
    rises (s < 0) over it"""
    a, b = oracle.carr_brute_trace(x, s, [at - 1, at])
    assert a != b, (x, s, at)
    return (b < a) if s > 0 else (b > a)


def on_lattice(gi):
    """rows whose whole chain stays on multiples of a power-of-two step (start 0 or 1 - 2^-53):
    its values land exactly on binade ends, where the walkers' conservative margins may leave the
    walked start itself out, and the segment then reports no interval (gss_spec_seg_walk)"""
    gi = np.asarray(gi).reshape(-1)
    a = np.abs(gi["s"])
    return (a > 0) & (np.frexp(a)[0] == 0.5) & ((gi["g"] == 0.0) | (gi["g"] == TOP))


def check_walks(gi, spec, n, may_void=None):
    """Every row with s != 0 against brute force.  Returns the number of translation checks made
    (d != 0 or d = 0 as an interval's end: at least two per segment with an interval).  A walked
    segment must report an interval, except in the rows of may_void (default: on_lattice)."""
    if may_void is None:
        may_void = on_lattice(gi)
    gi = np.asarray(gi).reshape(-1)
    spec = np.asarray(spec).reshape(-1)
    assert len(gi) == len(spec)
    checks = 0
    for r in np.flatnonzero(gi["s"] != 0):
        g, s, k = float(gi["g"][r]), float(gi["s"][r]), int(gi["k"][r])
        assert 1 <= k <= G.SPEC_K, (r, k)
        p1, w1 = int(spec["p1"][r]), float(spec["w1"][r])
        assert 0 < p1 <= n, (r, p1)
        if p1 < n:
            assert oracle.carr_brute(g, s, p1) == w1, (r, g, s, p1, w1)
            assert _wrapped(g, s, p1), (r, g, s, p1)
        unit = 2.0 ** -52 if s > 0 else 2.0 ** -53
        P, W = gi["P"][r], gi["W"][r]
        for j in range(k):
            sg = spec["seg"][r][j]
            dlo, dhi, end = float(sg["dlo"]), float(sg["dhi"]), float(sg["end"])
            pos, val = (p1, w1) if j == 0 else (int(P[j]), float(W[j]))
            stop = int(P[j + 1]) if j + 1 < k else n
            ln = stop - pos
            at = (r, j, val, s, ln, dlo, dhi)
            if ln <= 0:                                   # nothing to walk: no claim
                assert not dlo <= dhi, at
                continue
            assert 0.0 <= val < 1.0, at
            assert oracle.carr_brute(val, s, ln) == end, at
            assert int(sg["wrap_end"]) == int(_wrapped(val, s, ln)), at
            if not dlo <= dhi:                            # walked, and no interval claimed
                assert may_void[r], at
                continue
            assert dlo <= 0.0 <= dhi, at
            lo = math.ceil(max(dlo, -val) / unit) * unit         # the interval's ends on the
            hi = math.floor(min(dhi, 1.0 - unit - val) / unit) * unit    # lattice, inside [0, 1)
            assert lo <= 0.0 <= hi, at
            for d in sorted({lo, hi} | {u for u in (unit, -unit) if lo <= u <= hi}):
                assert 0.0 <= val + d < 1.0, at + (d,)
                assert oracle.carr_brute(val + d, s, ln) == end + d, at + (d,)
                checks += 1
    return checks


def _spec_walks_agree(got, want, gi, kw):
    """The device's walks against the host's (gss_spec_host): the same ends, wraps and first wraps
    bit for bit, and each segment's interval of exact start translations inside the host's (the
    device walks cycles from a cache its row's lanes share, whose entries' intervals are narrower:
    gss_producers.hip, sc_seg_walk); padding rows are not walked."""
    live = gi.reshape(-1)["s"] != 0
    assert np.array_equal(got["p1"][live], want["p1"][live]), kw
    assert np.array_equal(got["w1"][live], want["w1"][live]), kw
    narrower = 0
    for r in np.flatnonzero(live):
        k = gi.reshape(-1)["k"][r]
        g, w = got["seg"][r][:k], want["seg"][r][:k]
        assert g["end"].tobytes() == w["end"].tobytes(), (kw, r)
        assert np.array_equal(g["wrap_end"], w["wrap_end"]), (kw, r)
        empty = w["dlo"] > w["dhi"]                      # not walked: the same empty interval
        assert g[empty].tobytes() == w[empty].tobytes(), (kw, r)
        assert np.all(g["dlo"][~empty] >= w["dlo"][~empty]), (kw, r)
        assert np.all(g["dhi"][~empty] <= w["dhi"][~empty]), (kw, r)
        assert np.all(g["dlo"][~empty] <= 0) and np.all(g["dhi"][~empty] >= 0), (kw, r)
        narrower += int(np.sum((g["dlo"] != w["dlo"]) | (g["dhi"] != w["dhi"])))
    return narrower
