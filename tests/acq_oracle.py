"""A numpy restatement of the acquisition search (include/gpssim_amd.h, gss_acq_t; DESIGN.md
§12), independent of csrc/common/gss_acq.h: what gss_acquire_host and the GPU kernels are
compared with, bit for bit.  The correlator is a float64 matrix product of the Hankel matrix of
the quantised samples with the replicas; every sum stays below 2^53, so it is exact."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import gpssim_amd as G


def sizes(fs, coh_ms, M):
    L = fs * coh_ms // 1000
    T = -(-fs // 1000)
    E = -(-2 * fs // 1023000) + 1
    return L, T, M * L + T - 1, E


def unpack(samples, fmt, N):
    """(xI, xQ) int64[N] from the format's bytes"""
    b = np.ascontiguousarray(samples).view(np.uint8).reshape(-1)
    if fmt == 16:
        v = b[:4 * N].view("<i2").astype(np.int64)
    elif fmt == 8:
        v = b[:2 * N].view(np.int8).astype(np.int64)
    else:
        bits = np.unpackbits(b[:(2 * N + 7) // 8])[:2 * N]          # MSB first
        v = 2 * bits.astype(np.int64) - 1
    return v[0::2], v[1::2]


def auto_shift(xi, xq):
    v = 250 * (int(np.abs(xi).max()) + int(np.abs(xq).max()))
    sh = 0
    while (v >> sh) > 127:
        sh += 1
    return sh


def planes(xi, xq, fs, df, K, sh):
    """quantised wiped samples: (qI, qQ) int64 [2 K + 1, N]"""
    sin512, cos512 = (t.astype(np.int64) for t in G.lut())
    n = np.arange(len(xi), dtype=np.int64)
    qi, qq = [], []
    for k in range(-K, K + 1):
        step = ((k * df * 2**32 + fs // 2) // fs) % 2**32           # Python floor division
        idx = ((n * step) % 2**32) >> 23
        c, s = cos512[idx], sin512[idx]
        half = (1 << sh) >> 1
        qi.append(np.clip((xi * c + xq * s + half) >> sh, -127, 127))
        qq.append(np.clip((xq * c - xi * s + half) >> sh, -127, 127))
    return np.array(qi), np.array(qq)


def replicas(prns, fs, n, start=0):
    """+1 / -1 [len(prns), n]: replica samples start .. start + n - 1 (a negative index is the
    code continued backwards: floor division)"""
    ca = G.ca_table()
    chip = (np.arange(start, start + n, dtype=np.int64) * 1023000 // fs) % 1023
    out = np.empty((len(prns), n))
    for j, p in enumerate(prns):
        bit = (ca[p - 1][chip >> 5] >> (chip & 31).astype(np.uint32)) & 1
        out[j] = 2.0 * bit - 1.0
    return out


def acquire(samples, fs, fmt, coh_ms, M, K, df, prns, qshift=-1):
    """(peaks G.ACQ_PEAK_DTYPE [P], grid uint64 [P, 2 K + 1, T], resolved shift)"""
    prns = sorted(prns)
    L, T, N, E = sizes(fs, coh_ms, M)
    xi, xq = unpack(samples, fmt, N)
    sh = auto_shift(xi, xq) if qshift < 0 else qshift
    qi, qq = planes(xi, xq, fs, df, K, sh)
    rep = replicas(prns, fs, M * L)
    grid = np.zeros((len(prns), 2 * K + 1, T), np.uint64)
    for b in range(2 * K + 1):
        for m in range(M):
            r = rep[:, m * L:(m + 1) * L].T                          # [L, P]
            for q in (qi, qq):
                h = sliding_window_view(q[b, m * L:m * L + T + L - 1].astype(np.float64), L)
                s = (h @ r).astype(np.int64)                         # [T, P], exact
                grid[:, b, :] += (s * s).astype(np.uint64).T
    peaks = np.zeros(len(prns), G.ACQ_PEAK_DTYPE)
    t = np.arange(T)
    for j, p in enumerate(prns):
        best = int(np.argmax(grid[j].reshape(-1)))                   # first maximum: lowest k, tau
        kb, tau = divmod(best, T)
        d = np.abs(t - tau)
        far = np.minimum(d, T - d) > E
        peaks[j] = (grid[j, kb, tau], grid[j, kb][far].sum(dtype=np.uint64), int(far.sum()),
                    tau, kb - K, p)
    return peaks, grid, sh


def threshold_equation(M, x):
    """e^-x sum_{j < M} x^j / j!"""
    from math import exp, lgamma, log
    return sum(exp(-x + j * log(x) - lgamma(j + 1)) for j in range(M))


# ---- shared inputs ---------------------------------------------------------------------------
# (fs, coh_ms, M, K, df, PRNs): T = L = 64; tile edges in both dimensions and fs not a multiple
# of 1000; every slot of both column tiles with two windows; more than one chunk of L
SHAPES = [
    (64000, 1, 1, 2, 500, (1, 32)),
    (100010, 1, 3, 1, 500, (5, 6, 7)),
    (1000000, 2, 2, 3, 250, tuple(range(1, 33))),
    (2600000, 1, 1, 1, 500, (17, 28)),
]


def random_samples(fs, coh_ms, M, fmt, seed, extreme=False):
    """the bytes of N asymmetric random samples of a format (SC16: full range; extreme: every
    component at +32767 / -32768)"""
    N = sizes(fs, coh_ms, M)[2]
    rng = np.random.default_rng(seed)
    if fmt == 16:
        if extreme:
            v = np.where(rng.integers(0, 2, 2 * N) == 1, 32767, -32768).astype("<i2")
        else:
            v = rng.integers(-32768, 32768, 2 * N).astype("<i2")
        return v.view(np.uint8)
    if fmt == 8:
        return rng.integers(-128, 128, 2 * N).astype(np.int8).view(np.uint8)
    return rng.integers(0, 256, (N + 3) // 4 + 1).astype(np.uint8)


# ---- edge shapes, planted peaks and ties -----------------------------------------------------
# The correlator loads a window's q segment from the aligned dword below byte
# tau_blk + m L + i0 (tau_blk a multiple of 128, i0 of 1024) and adds the remainder shb to every
# later offset: shb != 0 needs L % 4 != 0, which no row of SHAPES has.
_ALL = tuple(range(1, 33))
EDGE_SHAPES = [
    (65001, 1, 3, 1, 500, (1, 32)),               # L = 65, T = 66: shb = 0, 1, 2; T below a tile
    (1023000, 1, 4, 1, 500, _ALL[:17]),           # L = T = 1023: shb = 0, 3, 2, 1; slot 16 alone
                                                  # in the second slot tile; one chunk of 1023
    (1025000, 1, 2, 0, 500, _ALL[:16]),           # L = T = 1025: a second chunk of one sample;
                                                  # 16 slots exactly; one bin; 8 tau tiles + 1
    (128000, 1, 2, 2, 500, (3,)),                 # L = T = 128: one full tau tile; one PRN
    (129000, 1, 1, 1, 500, (3, 9)),               # L = T = 129: one phase in a second tile
    (6000, 1, 1000, 1, 500, (1, 2)),              # L = T = 6: the smallest T (2 E + 1 = 5), the
                                                  # largest n_coh, one mostly-zero k-block
    (2047500, 2, 2, 1, 250, (1, 2, 3)),           # L = 4095, T = 2048: odd L over four chunks
                                                  # (the last of 1023); coh_ms 2; 16 tau tiles
    (6000, 1, 2, 130, 10, _ALL),                  # 261 bins: the peak kernel's second pass
    (1024000, 1, 2, 0, 500, (7,)),                # L = T = 1024: one full chunk, no zero padding
                                                  # of the replica; 8 tau tiles exactly
]
BINS261 = 7                                       # the row of EDGE_SHAPES with more than 256 bins
# the seed of a row's SC16 random input; BINS261's is chosen so that the peaks of the automatic
# shift lie on both sides of bin index 256 (checked by check_precondition)
_EDGE_SEED = {BINS261: 103}

PLANT_SHAPE = EDGE_SHAPES[1]
PLANT_TAUS = (0, 1, 3, 1019, 1021, 1022)          # 0, 1, E, T - 1 - E, T - 2, T - 1: the floor's
                                                  # excluded zone wraps at both ends


def planted(shape, taus, seed, amp=1000, noise=40):
    """SC16 bytes: the replica of the shape's j-th PRN delayed by taus[j] samples at amplitude amp
    on I, plus uniform noise of +- noise on I and Q"""
    fs, coh, M, _, _, prns = shape
    N = sizes(fs, coh, M)[2]
    v = np.random.default_rng(seed).integers(-noise, noise + 1, (N, 2))
    for p, tau in zip(sorted(prns), taus):
        v[:, 0] += amp * replicas([p], fs, N, start=-tau)[0].astype(np.int64)
    return v.astype("<i2").view(np.uint8).reshape(-1)


def half_rate(shape, tau, seed, amp=1000, noise=40):
    """SC16 bytes: the first PRN's replica delayed by tau, times (-1)^n.  With bin_hz = fs / 2
    the carrier steps of bins -1 and +1 are both 2^31, which undoes the alternation."""
    fs, coh, M, _, _, prns = shape
    N = sizes(fs, coh, M)[2]
    v = np.random.default_rng(seed).integers(-noise, noise + 1, (N, 2))
    sign = 1 - 2 * (np.arange(N) & 1)
    v[:, 0] += amp * sign * replicas([sorted(prns)[0]], fs, N, start=-tau)[0].astype(np.int64)
    return v.astype("<i2").view(np.uint8).reshape(-1)


def constant(shape):
    """SC16 bytes: xI = 1, xQ = 0"""
    N = sizes(*shape[:3])[2]
    return np.tile(np.array([1, 0], "<i2"), N).view(np.uint8)


def edge_cases():
    """(name, shape, fmt, (kind, seed), qshift) for every row of EDGE_SHAPES: SC16 at shift 0, 7
    and automatic and the extreme input; SC08 and SC01 at the automatic shift and at 0 (SC08 at
    0: already-quantised samples times 250, every sum saturated)"""
    out = []
    for si, s in enumerate(EDGE_SHAPES):
        for q in (0, 7, -1):
            out.append((f"e{si}-q{q}", s, 16, ("rand", _EDGE_SEED.get(si, 100 + si)), q))
        out.append((f"e{si}-extreme", s, 16, ("extreme", 150 + si), -1))
        for fmt in (8, 1):
            for q in (-1, 0):
                out.append((f"e{si}-b{fmt}-q{q}", s, fmt, ("rand", 120 + si), q))
    return out


# Ties.  bin_hz = fs makes every carrier step 0 mod 2^32 (all bins of a PRN identical);
# bin_hz = fs / 2 with K = 1 makes bins -1 and +1 identical; a constant input with one bin makes
# a whole row equal and non-zero.  The sine table is not symmetric: mirror bins do not tie.
SPECIAL_CASES = [
    ("planted", PLANT_SHAPE, 16, ("planted", 5), -1),
    ("alias-64", (64000, 1, 2, 2, 64000, (1, 32)), 16, ("rand", 200), -1),
    ("alias-261", (6000, 1, 2, 130, 6000, _ALL), 16, ("rand", 201), -1),
    ("half-rate", (64000, 1, 2, 1, 32000, (1, 32)), 16, ("half", 202), -1),
    ("const-64", (64000, 1, 2, 0, 500, (1, 32)), 16, ("const", 0), 0),
    ("const-1025", (1025000, 1, 2, 0, 500, (1, 17, 32)), 16, ("const", 0), 0),
    ("zero", SHAPES[0], 16, ("zero", 0), 0),
]
HALF_TAU = 37


def case_data(case):
    """the input bytes of a case of edge_cases() or SPECIAL_CASES"""
    _, shape, fmt, (kind, seed), _ = case
    if kind == "planted":
        return planted(shape, PLANT_TAUS, seed)
    if kind == "half":
        return half_rate(shape, HALF_TAU, seed)
    if kind == "const":
        return constant(shape)
    if kind == "zero":
        return np.zeros(4 * sizes(*shape[:3])[2], np.uint8)
    return random_samples(shape[0], shape[1], shape[2], fmt, seed, extreme=kind == "extreme")


_answers = {}


def answer(case):
    """acquire() over a case's input, computed once per process: the host tests and both GPU
    paths share it.  What the case is for is checked here, on the oracle's own answer."""
    name, shape, fmt, _, qshift = case
    if name not in _answers:
        fs, coh, M, K, df, prns = shape
        _answers[name] = acquire(case_data(case), fs, fmt, coh, M, K, df, prns, qshift)
        check_precondition(case, *_answers[name][:2])
    return _answers[name]


def check_precondition(case, peaks, grid):
    """does the oracle's answer show the edge the case was built for?"""
    name, shape, _, (kind, _), _ = case
    K, T = shape[3], grid.shape[2]
    if kind == "planted":                          # every planted PRN peaks where it was put
        n = len(PLANT_TAUS)
        assert tuple(peaks["tau"][:n]) == PLANT_TAUS and (peaks["bin"][:n] == 0).all(), peaks
    elif name.startswith("alias"):                 # identical bins: bin -K, the first maximum
        assert (grid == grid[:, :1, :]).all() and grid.any()
        assert (peaks["bin"] == -K).all()
        assert (peaks["tau"] == grid[:, 0, :].argmax(axis=1)).all()
    elif kind == "half":                           # the peak in the tied pair: the lower bin
        assert np.array_equal(grid[:, 0], grid[:, 2])
        assert peaks["bin"][0] == -1 and peaks["tau"][0] == HALF_TAU, peaks
        assert grid[0, 0].max() > grid[0, 1].max()
    elif kind == "const":                          # one equal non-zero row per PRN: tau 0
        assert (grid == grid[:, :, :1]).all() and grid.all()
        assert (peaks["tau"] == 0).all() and (peaks["bin"] == 0).all()
        assert (peaks["floor_cnt"] == T - 2 * sizes(*shape[:3])[3] - 1).all()
    elif kind == "zero":
        assert not grid.any() and (peaks["tau"] == 0).all() and (peaks["bin"] == -K).all()
    elif name == f"e{BINS261}-q-1":                # peaks in both passes of the candidate loop
        idx = peaks["bin"] + K
        assert (idx >= 256).any() and (idx < 256).any(), idx


# ---- the physical test's inputs --------------------------------------------------------------
# Block 0 of the static 1 s scenario at 1 MS/s, rendered by the CPU oracle from Scenario.next
# rows, with noise at 50 dB-Hz (sigma = 250 sqrt(fs / (2 * 10^(cn0 / 10))), seed 7); the noise
# option's shift is 0 for SC16 and SC01 and 2 for SC08 (the CLI's automatic choice there).
PHYS_FS = 1000000
PHYS_CN0 = 50.0
PHYS_K, PHYS_DF, PHYS_M = 10, 500, 8
ABSENT = (4, 5, 7, 8)
_blocks = {}


def PHYS_ACQ(fmt):
    return G.Acq(PHYS_FS, fmt, 1, PHYS_M, PHYS_DF, PHYS_K, -1)


def phys_threshold(M=PHYS_M):
    return G.acq_threshold(M, (2 * PHYS_K + 1) * 1000, 1e-3)


def noisy_block(fmt, clean=False):
    """(bytes of block 0 in format fmt, its rows blk[1, 16], nch[1]); computed once"""
    from conftest import LOC, NAV
    import oracle
    if "rows" not in _blocks:
        s = G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=float(PHYS_FS))
        blk, nch = s.next(1)
        out, rc = oracle.synth(blk, nch, G.ca_table(), s.nav_table(), s.n_per_blk, 16)
        assert rc == 0
        _blocks["rows"] = (blk, nch)
        _blocks["iq"] = out.view(np.int16).copy()
        s.close()
    blk, nch = _blocks["rows"]
    key = (fmt, clean)
    if key not in _blocks:
        sigma = 0 if clean else int(np.floor(
            256 * 250 * np.sqrt(PHYS_FS / (2 * 10 ** (PHYS_CN0 / 10))) + 0.5))
        shift = 2 if (fmt == 8 and not clean) else 0
        _blocks[key] = G.impair_host(G.Impair(sigma, shift, 7), _blocks["iq"], 0, fmt)
    return _blocks[key], blk, nch


def check_physical(peaks, blk, nch, level, found=True, M=PHYS_M):
    """every row of the block is located within one sample and one bin (and, found: detected at
    pfa 1e-3, the absent PRNs not); level: the C/N0 estimate within 3 dB of what was asked for,
    corrected for the row's gain, the code-phase offset and the Doppler offset"""
    by_prn = {int(p["prn"]): p for p in peaks}
    thr = phys_threshold(M)
    T = 1000
    rows = blk[0][:nch[0]]
    assert len(rows) == 11
    for row in rows:
        t = G.acq_expect(row, PHYS_FS, 0)
        p = by_prn[t["prn"]]
        dt = abs(p["tau"] - t["tau"]) % T
        dt = min(dt, T - dt)
        dfq = p["bin"] * PHYS_DF - t["doppler_hz"]
        ratio = G.acq_ratio(p)
        print(t["prn"], p["tau"], t["tau"], dfq, ratio)
        assert dt <= 1, (t, p)
        assert abs(dfq) <= PHYS_DF, (t, p)
        if found:
            assert ratio >= thr, (t, p, ratio, thr)
        if level:
            want = (PHYS_CN0 + t["cn0_offset_db"] + 20 * np.log10(1 - dt * 1023000 / PHYS_FS)
                    + 20 * np.log10(abs(np.sinc(dfq * 1e-3))))
            print("   cn0", G.cn0_dbhz(p), want)
            assert abs(G.cn0_dbhz(p) - want) <= 3.0, (t, p, G.cn0_dbhz(p), want)
    if found:
        present = {G.acq_expect(r, PHYS_FS, 0)["prn"] for r in rows}
        for a in ABSENT:
            assert a not in present and G.acq_ratio(by_prn[a]) < thr, a
