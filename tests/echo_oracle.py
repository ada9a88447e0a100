"""Restatement of the multipath-echo definition (include/gpssim_amd.h, gss_echo_t), independent
of the library: the carrier tables come from tests/golden/lut512.json (the reference's own), a
pair's integers are Python integers made from the row's doubles with the definition's own IEEE
operations, the per-sample terms are numpy int64 / uint64 (whose array arithmetic wraps mod 2^64)
and are checked on every call against plain Python integers at the ends and at a few hundred
samples between.  Rows come from exact_oracle.rows().  Shared by tests/test_echo.py and
tests/test_gpu_echo.py."""
import functools
import math

import numpy as np

import exact_oracle as X
import gpssim_amd as G
from impair_oracle import samples
from jam_oracle import tables

M64 = (1 << 64) - 1
DELAY_END = 1023 << 32
U = np.uint64


def E(delay=0, theta0=0, dstep=0, alpha_q16=65536, prn=0):
    """an echo as a dict of Python integers (theta0, dstep mod 2^64)"""
    return dict(delay=delay, theta0=theta0 & M64, dstep=dstep & M64, alpha_q16=alpha_q16, prn=prn)


def to_echo(e):
    return G.Echo(**e)


def in_range(row):
    """the row's doubles lie where the definition's conversions are defined (NaN: nowhere)"""
    return bool(0.0 <= float(row["carr0"]) <= 1.0 and -1.0 < float(row["carr_step"]) < 1.0 and
                0.0 <= float(row["code0"]) < 1023.0 and 0.0 <= float(row["code_step"]) < 1024.0)


def live(e, row, n_ca, n_nav):
    t = int(row["ca_tbl"])
    return (0 <= t < n_ca and 0 <= int(row["nav_tbl"]) < n_nav and in_range(row) and
            (e["prn"] == 0 or e["prn"] == t + 1))


def contributes(e, row, n_ca, n_nav):
    """live, and with a gain that is not zero: the pair reaches its block's samples"""
    return live(e, row, n_ca, n_nav) and ints(e, row)[4] != 0


def ints(e, row):
    """the pair's integers (P0, Ps, X0, Cs, g), Python integers"""
    carr0, cstep = float(row["carr0"]), float(row["carr_step"])
    P0 = 0 if carr0 >= 1.0 else int(carr0 * 2.0 ** 64)
    Ps = (2 * int(math.trunc(cstep * 2.0 ** 63))) & M64
    C0 = int(math.floor(float(row["code0"]) * 2.0 ** 32))
    Cs = int(math.floor(float(row["code_step"]) * 2.0 ** 32 + 0.5))
    per = ((int(row["iword"]) * 30 + int(row["ibit"])) * 20 + int(row["icode"])) * 1023
    X0 = (per << 32) + C0 - e["delay"]
    g = (int(row["gain"]) * e["alpha_q16"] + (1 << 15)) >> 16
    return P0, Ps, X0, Cs, max(-32767, min(32767, g))


def value_py(e, row, ca, nav, s, a):
    """(E_I, E_Q) term of one live pair at sample s of its block, absolute index a"""
    P0, Ps, X0, Cs, g = ints(e, row)
    q = (X0 + s * Cs) >> 32
    chip, cp = q % 1023, max(q // 1023, 0)
    bit = cp // 20
    word, pos = min(bit // 30, 59), bit % 30
    c = 2 * ((int(ca[row["ca_tbl"]][chip // 32]) >> (chip % 32)) & 1) - 1
    d = 2 * ((int(nav[row["nav_tbl"]][word]) >> (29 - pos)) & 1) - 1
    idx = ((P0 + s * Ps + e["theta0"] + a * e["dstep"]) & M64) >> 55
    cos, sin = tables()
    return d * c * int(cos[idx]) * g, d * c * int(sin[idx]) * g


def pair_terms(e, row, ca, nav, n, base):
    """int64[n, 2]: the pair's terms over its block, whose first sample has absolute index base"""
    P0, Ps, X0, Cs, g = ints(e, row)
    assert -2 ** 63 <= X0 + (n - 1) * Cs < 2 ** 63 and -2 ** 63 <= X0 < 2 ** 63
    s = np.arange(n, dtype=np.int64)
    q = (np.int64(X0) + s * np.int64(Cs)) >> np.int64(32)
    chip = q % 1023
    cp = np.maximum(q // 1023, 0)
    bit = cp // 20
    word, pos = np.minimum(bit // 30, 59), bit % 30
    cw = ca[int(row["ca_tbl"])].astype(np.int64)[chip >> 5]
    c = 2 * ((cw >> (chip & 31)) & 1) - 1
    nw = nav[int(row["nav_tbl"])].astype(np.int64)[word]
    d = 2 * ((nw >> (29 - pos)) & 1) - 1
    su = s.astype(np.uint64)
    phi = U((P0 + e["theta0"] + base * e["dstep"]) & M64) + su * U((Ps + e["dstep"]) & M64)
    idx = (phi >> U(55)).astype(np.int64)
    cos, sin = tables()
    return np.stack([d * c * cos[idx] * g, d * c * sin[idx] * g], axis=-1)


def echo(echoes, blk, nch, ca, nav, n, sample0, iq):
    """int16[2 nblk n]: iq with the echoes of the rows added"""
    x = np.asarray(iq, np.int16).reshape(-1, 2).astype(np.int64)
    nblk = len(nch)
    assert x.shape[0] == nblk * n and sample0 + nblk * n <= 1 << 64
    ca, nav = np.asarray(ca, np.uint32).reshape(-1, 32), np.asarray(nav, np.uint32).reshape(-1, 60)
    acc = np.zeros_like(x)
    for b in range(nblk):
        for e in echoes:
            for k in range(int(nch[b])):
                if live(e, blk[b, k], len(ca), len(nav)):
                    acc[b * n:(b + 1) * n] += pair_terms(e, blk[b, k], ca, nav, n, sample0 + b * n)
    assert np.abs(acc).max(initial=0) < 1 << 30
    y = np.clip(x + ((acc + 64) >> 7), -32768, 32767)
    N = nblk * n
    for i in sorted({0, 1, N - 2, N - 1, *range(0, N, max(1, N // 257))} & set(range(N))):
        b, s = divmod(i, n)
        want = [0, 0]
        for e in echoes:
            for k in range(int(nch[b])):
                if live(e, blk[b, k], len(ca), len(nav)):
                    t = value_py(e, blk[b, k], ca, nav, s, sample0 + i)
                    want = [want[0] + t[0], want[1] + t[1]]
        assert [int(v) for v in acc[i]] == want, (i, b, s)
    return y.astype(np.int16).reshape(-1)


# ---- gss_echo_make's formulas, the same IEEE double operations -----------------------------------
def make(fs, prn, delay_m, atten_db, phase_deg=0.0, doppler_hz=0.0):
    t = phase_deg / 360.0
    th = (t - math.floor(t)) * 2.0 ** 64
    return E(delay=int(math.floor(delay_m * 1023000.0 / 299792458.0 * 4294967296.0 + 0.5)),
             alpha_q16=int(math.floor(65536.0 * math.pow(10.0, -atten_db / 20.0) + 0.5)),
             theta0=0 if th >= 2.0 ** 64 else int(th),
             dstep=int(math.floor(doppler_hz / fs * 2.0 ** 64 + 0.5)), prn=prn)


# ---- the cases both test files run ---------------------------------------------------------------
SIZES = [1, 2, 3, 7, 33, 1023, 1025, 4099]
STARTS = [0, 1, 2 ** 32 - 5, 2 ** 40 + 3]
DELAYS = [0, 1, 2 ** 31, 2 ** 32 + 1, DELAY_END - 1]
HI = 0xF123456789ABCDEF
# rows cycle through (icode, ibit, iword): seeded draws, the frame's first period (a delay reaches
# before it where code0 is 0) and its last (the code runs past word 59)
COUNTERS = [None, (0, 0, 0), (19, 29, 59), None, None]
CARR_STEPS = [c for c in X.CARR_STEPS if abs(c) < 0.5]
NO_PRN = 32                                            # tables() below never uses C/A row 31


def _tables(seed):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, 31)), int(rng.integers(0, 8))) for _ in range(37)]


def four(prn=0):
    """four echoes: the delays 2^31, 1023 * 2^32 - 1, 2^32 + 1 and 1, dstep of both signs and 0,
    alpha 1/2, 1, 4 and 0.3"""
    return [E(DELAYS[2], 1 << 62, 12345 << 20, 32768, prn), E(DELAYS[4], HI, -(777 << 30), 65536, prn),
            E(DELAYS[3], 0, HI, 1 << 18, prn), E(DELAYS[1], 5, 0, 20000, prn)]


def sets(blk, nch):
    """the echo sets of one case: none; one on every channel; one without delay on the PRN of a
    row, one on a PRN no row has and a silent one (alpha 0) on every channel; four on every channel
    (64 pairs with 16 channels)"""
    some = [int(blk[b, 0]["ca_tbl"]) + 1 for b in range(len(nch)) if nch[b] > 0]
    prn = some[0] if some else 1
    return [[], [E(DELAYS[2], 3 << 61, -(1 << 50), 40000, 0)],
            [E(DELAYS[0], 0, 1 << 40, 65536, prn), E(DELAYS[3], 1 << 63, 1 << 40, 30000, NO_PRN),
             E(DELAYS[1], 5, 77, 0, 0)], four()]


@functools.lru_cache(maxsize=None)
def ca_table():
    return G.ca_table()


def case(n, nchs, seed, gain=X.GAINS):
    blk, nch, nav = X.rows(nchs, X.CODE_STEPS, CARR_STEPS, gain=gain, counters=COUNTERS,
                           carr0=X.CARR0S, code0=[0.0, None, 1022.9999999, None],
                           tables=_tables(seed), seed=seed)
    return blk, nch, nav


NCHS = [[16, 0, 5, 1, 16], [5, 16, 1], [1, 5, 16, 0], [16, 16, 16], [0, 0, 0]]


def cases():
    """(name, echoes, blk, nch, nav, n, sample0, iq): every size with 3 to 5 blocks and channel
    counts 0, 1, 5 and 16, every echo set; the start moves with the row set and with the echo set
    (16 row sets, 4 echo sets, 4 starts: every echo set meets every start); then the clamps and
    the rows outside the definition's range"""
    out = []
    i = 0
    for c, (n, half) in enumerate((n, half) for n in SIZES for half in (0, 1)):
        nchs = NCHS[(c + c // len(NCHS)) % len(NCHS)]
        blk, nch, nav = case(n, nchs, seed=100 + c)
        for k, es in enumerate(sets(blk, nch)):
            s0 = STARTS[(c + k) % len(STARTS)]
            out.append((f"n{n}_c{len(out)}", es, blk, nch, nav, n, s0,
                        samples(len(nch) * n, seed=i)))
            i += 1
    # the clamp on g (|gain| alpha >> 16 past 32767) and, through it, int16 on both rails
    blk, nch, nav = case(1025, [5, 16, 1], seed=7, gain=[20000, -20000, 12000, -8191, 8192])
    for a in (0, 65536, 1 << 18):
        out.append((f"clamp_a{a}", [E(DELAYS[2], 0, 1 << 45, a, 0)], blk, nch, nav, 1025, 2 ** 32 - 5,
                    samples(3 * 1025, seed=a)))
    # 64 pairs that all reach the samples: 16 channels, no gain that an alpha rounds to 0
    blk, nch, nav = case(1025, [16, 16, 16], seed=8, gain=[97, -64, 129, 500, 33, -250, 7])
    out.append(("pairs64", four(), blk, nch, nav, 1025, 2 ** 40 + 3, samples(3 * 1025, seed=22)))
    # rows whose doubles lie outside the definition's range add nothing; their neighbours do
    blk, nch, nav = case(1025, [5, 16, 1], seed=9)
    blk = blk.copy()
    for k, (f, v) in enumerate([("carr0", float("nan")), ("carr0", -0.25), ("carr0", 1.5),
                                ("carr_step", 1.0), ("carr_step", -1e300), ("code0", 1023.0),
                                ("code0", -1.0), ("code_step", 1024.0), ("code_step", float("inf")),
                                ("code_step", -0.5), ("carr_step", float("nan"))]):
        blk[1, k][f] = v
    out.append(("rows_out_of_range", four(), blk, nch, nav, 1025, 1, samples(3 * 1025, seed=21)))
    return out


def run_host(c):
    _, es, blk, nch, nav, n, s0, iq = c
    return G.echo_host([to_echo(e) for e in es], blk, nch, ca_table(), nav, n, s0, iq)


@functools.lru_cache(maxsize=None)
def want(i):
    """the oracle's bytes of cases()[i], computed once"""
    _, es, blk, nch, nav, n, s0, iq = cases_cached()[i]
    w = echo(es, blk, nch, ca_table(), nav, n, s0, iq)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def cases_cached():
    return cases()
