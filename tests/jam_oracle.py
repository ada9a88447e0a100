"""Restatement of the jammer definition (include/gpssim_amd.h, gss_jam_t), independent of the
library: the carrier tables come from tests/golden/lut512.json (the reference's own), the
constants of a sweep are Python integers, the per-sample phases are numpy uint64 (whose array
arithmetic wraps mod 2^64) and are checked on every call against plain Python integers at the
ends and at a few hundred samples between.  The noise, the level and the formats are those of
tests/impair_oracle.py.  Shared by tests/test_jam.py and tests/test_gpu_jam.py."""
import json
import math
import os

import numpy as np

import impair_oracle as IO

M64 = (1 << 64) - 1
_LUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lut512.json")
_tables = None


def tables():
    """(cos512, sin512) int64[512]"""
    global _tables
    if _tables is None:
        d = json.load(open(_LUT))
        _tables = (np.array(d["cosTable512"], np.int64), np.array(d["sinTable512"], np.int64))
        assert _tables[0].shape == _tables[1].shape == (512,)
    return _tables


def J(step0=0, rate=0, phase0=0, sweep=1, amp=65536, gate_period=0, gate_on=0, gate_shift=0):
    """a jammer as a dict of Python integers (step0, rate, phase0 mod 2^64)"""
    return dict(step0=step0 & M64, rate=rate & M64, phase0=phase0 & M64, sweep=sweep, amp=amp,
                gate_period=gate_period, gate_on=gate_on, gate_shift=gate_shift)


def phase_py(j, n):
    """Phi of absolute sample n, Python integers"""
    P = j["sweep"]
    k, m = divmod(n, P)
    phip = P * j["step0"] + j["rate"] * (P * (P - 1) // 2)
    return (j["phase0"] + k * phip + m * j["step0"] + j["rate"] * (m * (m - 1) // 2)) & M64


def on_py(j, n):
    gp = j["gate_period"]
    return gp == 0 or ((n % gp) + j["gate_shift"]) % gp < j["gate_on"]


def value_py(j, n):
    """(jI, jQ) of absolute sample n, Python integers"""
    if not on_py(j, n):
        return 0, 0
    c, s = tables()
    idx = phase_py(j, n) >> 55
    return (j["amp"] * int(c[idx]) + (1 << 15)) >> 16, (j["amp"] * int(s[idx]) + (1 << 15)) >> 16


def jam_iq(j, sample0, n):
    """int64[n, 2]: (jI, jQ) of samples sample0 .. sample0 + n - 1"""
    assert 0 <= sample0 and sample0 + n <= 1 << 64
    U = np.uint64
    idx = np.arange(n, dtype=np.uint64) + U(sample0)
    P = j["sweep"]
    k, m = idx // U(P), idx % U(P)
    phip = (P * j["step0"] + j["rate"] * (P * (P - 1) // 2)) & M64
    tri = (m * (m - U(1) + (m == 0).astype(np.uint64))) >> U(1)      # m (m - 1) / 2 < 2^63; 0 at m = 0
    phi = U(j["phase0"]) + k * U(phip) + m * U(j["step0"]) + U(j["rate"]) * tri
    gp = j["gate_period"]
    if gp:
        on = ((idx % U(gp)) + U(j["gate_shift"])) % U(gp) < U(j["gate_on"])
    else:
        on = np.ones(n, bool)
    c, s = tables()
    cell = (phi >> U(55)).astype(np.int64)
    out = np.stack([(j["amp"] * c[cell] + (1 << 15)) >> 16, (j["amp"] * s[cell] + (1 << 15)) >> 16],
                   axis=-1)
    out[~on] = 0
    for i in sorted({0, 1, n - 2, n - 1, *range(0, n, max(1, n // 257))} & set(range(n))):
        assert int(phi[i]) == phase_py(j, sample0 + i), (j, sample0 + i)
        assert tuple(int(v) for v in out[i]) == value_py(j, sample0 + i), (j, sample0 + i)
    return out


def jam(seed, sigma_q8, shift, jams, iq, sample0, fmt, g=None):
    """the bytes (uint8) of format fmt for jammer-free, noise-free iq int16[2 n] from sample0 on"""
    x = np.asarray(iq, np.int16).reshape(-1, 2).astype(np.int64)
    n = len(x)
    v = x.copy()
    for j in jams:
        v += jam_iq(j, sample0, n)
    if g is None:
        g = IO.noise(seed, sigma_q8, sample0, n) if sigma_q8 else 0
    w = (v + g + ((1 << shift) >> 1)) >> shift
    if fmt == 16:
        return np.clip(w, -32768, 32767).astype(np.int16).reshape(-1).view(np.uint8)
    if fmt == 8:
        return np.clip(w >> 4, -128, 127).astype(np.int8).reshape(-1).view(np.uint8)
    assert fmt == 1 and n % 4 == 0
    return np.packbits((w > 0).astype(np.uint8).reshape(-1))


# ---- gss_jam_make's formulas, the same IEEE double operations -----------------------------------
def step_of(f, fs):
    return int(math.floor(f / fs * 18446744073709551616.0 + 0.5))


def make(fs, js_db, f0, f1=0.0, sweep_s=0.0, gate_period_s=0.0, duty=0.0):
    amp = int(math.floor(65536.0 * math.pow(10.0, js_db / 20.0) + 0.5))
    j = J(step0=step_of(f0, fs), amp=amp)
    if sweep_s:
        P = int(math.floor(sweep_s * fs + 0.5))
        j["sweep"] = P
        j["rate"] = ((step_of(f1, fs) - step_of(f0, fs)) // P) & M64       # floored
    if gate_period_s:
        gp = math.floor(gate_period_s * fs + 0.5)
        j["gate_period"] = int(gp)
        j["gate_on"] = int(math.floor(duty * gp + 0.5))
    return j


# ---- the cases both test files run --------------------------------------------------------------
HI = 0xF123456789ABCDEF                                # a step with its high bits set
CW = [J(step0=step_of(137e3, 1e6)), J(step0=-step_of(137e3, 1e6), phase0=1 << 62), J(step0=HI)]


def sweeps(P):
    """a sweep of P samples, and one whose rate takes the step past 2^63 inside it"""
    return [J(step0=-(1 << 62), rate=((1 << 63) // max(P, 2)) | 1, sweep=P, phase0=12345 << 40),
            J(step0=(1 << 63) - 5, rate=(1 << 61) + 7, sweep=P)]


GATES = [dict(gate_period=1, gate_on=0), dict(gate_period=1, gate_on=1),
         dict(gate_period=10, gate_on=3, gate_shift=0), dict(gate_period=10, gate_on=3, gate_shift=9),
         dict(gate_period=7, gate_on=0), dict(gate_period=7, gate_on=7),
         dict(gate_period=3, gate_on=2, gate_shift=1)]
SWEEP_P = [1, 2, 3, 7, 137, 2**32 - 1]
SIZES = [4, 36, 4100]
STARTS = [0, 1, 2**32 - 5, 2**40 + 3, 2**64 - 4100]
NOISE = [(0, 0), (256 * 300, 1)]                       # (sigma_q8, shift)


def four(P=137):
    """four jammers: a tone, a gated tone, a sweep, a gated fast sweep"""
    return [CW[0], dict(CW[1], **GATES[3], amp=3 * 65536), sweeps(P)[0],
            dict(sweeps(3)[1], **GATES[6], amp=1 << 20)]


def cases():
    """(jammers, extra starts): the tones, every sweep length with a start three samples before
    a wrap, the gates, the levels, none and four"""
    out = [([], []), (four(), [5 * 137 - 3])]
    out += [([j], []) for j in CW]
    for P in SWEEP_P:
        out += [([j], [5 * P - 3]) for j in sweeps(P)]
    out += [([dict(CW[0], **g)], []) for g in GATES]
    out += [([dict(sweeps(7)[0], **GATES[2])], [7 * 10 - 3])]
    return out


def to_jam(G, j):
    return G.Jam(**j)
