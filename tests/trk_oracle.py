"""A numpy restatement of the tracking loops (include/gpssim_amd.h, gss_trk_cfg_t),
independent of csrc/common/gss_trk.h: what gss_track_host and the GPU kernel are compared with,
bit for bit.  The samples of an epoch are correlated as int64 vectors; the state is Python
integers, wrapped by hand where the definition wraps."""
import numpy as np

import gpssim_amd as G
from acq_oracle import unpack

M = 1023 << 32
HALF = 1 << 31


def tdiv(a, b):
    """C's truncating division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def amb(a, b):
    a, b = abs(a), abs(b)
    return max(a, b) + (min(a, b) >> 1)


def cs_nominal(fs):
    return (1023000 * 2**32 + fs // 2) // fs


def defaults(fs):
    """(n_pull, Kf, Ki, Kp, Kd) of gss_trk_defaults"""
    from math import floor, pi
    T, wn = 1e-3, 34.0
    return (300, floor(0.05 * 2**34 / (2 * pi * T * fs) + 0.5),
            floor(wn * wn * T * 2**34 / (2 * pi * fs) + 0.5),
            floor(1.414 * wn * 2**34 / (2 * pi * fs) + 0.5), floor(8 * 2**33 / fs + 0.5))


def track(samples, fmt, N, fs, gains, jobs, pitch):
    """(rec G.TRK_REC_DTYPE [n_job, pitch], count int32 [n_job]); gains = (n_pull, Kf, Ki, Kp,
    Kd), jobs = [(prn, s0, w0, n_epoch)]"""
    n_pull, Kf, Ki, Kp, Kd = gains
    xi, xq = unpack(samples, fmt, N)
    sin512, cos512 = (t.astype(np.int64) for t in G.lut())
    ca = G.ca_table()
    cs_nom = cs_nominal(fs)
    rec = np.zeros((len(jobs), pitch), G.TRK_REC_DTYPE)
    count = np.zeros(len(jobs), np.int32)
    for j, (prn, s0, w0, n_epoch) in enumerate(jobs):
        row = ca[prn - 1]
        chips = 2 * ((row[np.arange(1023) >> 5] >> (np.arange(1023) & 31).astype(np.uint32))
                     & 1).astype(np.int64) - 1
        s, phi, th, w, W = s0, 0, 0, w0, w0 << 16
        cs = cs_nom + tdiv(w0, 1540)
        up = vp = 0
        for e in range(n_epoch):
            n = -(-(M - phi) // cs)
            if s + n > N:
                break
            i = np.arange(n, dtype=np.int64)
            c = phi + i * cs
            idx = ((th + i * w) % 2**32) >> 23
            co, si = cos512[idx], sin512[idx]
            x, y = xi[s:s + n], xq[s:s + n]
            yi, yq = x * co + y * si, y * co - x * si
            E, P, L = (chips[k >> 32] for k in ((c + HALF) % M, c, (c - HALF) % M))
            IE, QE, IP, QP, IL, QL = (int((a * b).sum()) for b in (E, P, L) for a in (yi, yq))
            rec[j, e] = (IE, QE, IP, QP, IL, QL, s, w, cs - cs_nom)
            m = amb(IP, QP)
            u = tdiv(IP << 14, m) if m else 0
            v = tdiv(QP << 14, m) if m else 0
            d_pll = -v if u < 0 else v
            d_fll = 0
            if e > 0:
                cross, dot = up * v - vp * u, up * u + vp * v
                d_fll = (-cross if dot < 0 else cross) >> 14
            mE, mL = amb(IE, QE), amb(IL, QL)
            d_dll = tdiv((mE - mL) << 14, mE + mL) if mE + mL else 0
            th = (th + n * w) % 2**32
            phi += n * cs - M
            s += n
            if e < n_pull:
                W = s64(W + Kf * d_fll)
                w = s32(W >> 16)
            else:
                W = s64(W + Ki * d_pll)
                w = s32((W + Kp * d_pll) >> 16)
            cs = cs_nom + tdiv(w, 1540) + ((Kd * d_dll) >> 16)
            up, vp = u, v
            count[j] = e + 1
    return rec, count


# ---- shared inputs ---------------------------------------------------------------------------
# (fs, epochs, n_pull, [(prn, s0, w0)]): an epoch shorter than a workgroup; epoch lengths that
# alternate; the bench rate.  n_pull lies inside every run, so both filter branches execute, and
# the last job of each shape starts so late that it runs out of samples inside an epoch.
def _w(hz, fs):
    return s32((hz * 2**32 + fs // 2) // fs)


def shapes():
    out = []
    for fs, ne in ((64000, 60), (100010, 50), (2600000, 40)):
        T = -(-fs // 1000)
        N = ne * fs // 1000 + T + 7
        jobs = [(1, 3, _w(1234, fs), ne), (17, T // 2 + 1, _w(-2750, fs), ne - 5),
                (32, N - 9 * fs // 1000 - T // 3, _w(40, fs), ne)]
        out.append((fs, N, 25, jobs))
    return out


SHAPES = shapes()


def random_samples(N, fmt, seed):
    """the bytes of N asymmetric random samples of a format (SC16: the full range)"""
    rng = np.random.default_rng(seed)
    if fmt == 16:
        return rng.integers(-32768, 32768, 2 * N).astype("<i2").view(np.uint8)
    if fmt == 8:
        return rng.integers(-128, 128, 2 * N).astype(np.int8).view(np.uint8)
    return rng.integers(0, 256, (N + 3) // 4).astype(np.uint8)


def gains_of(fs, n_pull):
    return (n_pull,) + defaults(fs)[1:]


def trk_of(fs, fmt, gains):
    return G.Trk(fs, fmt, n_pull=gains[0], Kf=gains[1], Ki=gains[2], Kp=gains[3], Kd=gains[4])


def jobs_array(jobs):
    a = np.zeros(len(jobs), G.TRK_JOB_DTYPE)
    for k, (prn, s0, w0, ne) in enumerate(jobs):
        a[k] = (s0, prn, w0, ne, 0)
    return a


_want = {}


def want(si, fmt, seed):
    """the oracle's answer for shape si, computed once: (samples, rec, count)"""
    key = (si, fmt, seed)
    if key not in _want:
        fs, N, n_pull, jobs = SHAPES[si]
        data = random_samples(N, fmt, seed)
        pitch = max(j[3] for j in jobs)
        _want[key] = (data,) + track(data, fmt, N, fs, gains_of(fs, n_pull), jobs, pitch)
    return _want[key]


def same_records(rec, count, wrec, wcount):
    """the records written equal the oracle's, count for count"""
    assert np.array_equal(count, wcount), (count, wcount)
    for j, c in enumerate(wcount):
        bad = np.nonzero(rec[j, :c] != wrec[j, :c])[0]
        assert len(bad) == 0, (j, bad[:4], rec[j, bad[:1]], wrec[j, bad[:1]])


# ---- input families --------------------------------------------------------------------------
# Synthetic inputs that reach what the shapes above do not: every epoch length at which the fast
# form of the kernel takes another path, the int32 partial sums at their limit, the feedback at
# the ends of its arguments, and jobs that end exactly where the samples do.  A case is a dict
# (fs, fmt, N, gains, jobs, pitch, data, rec, count), built with the oracle's answer on first use
# (case(name)) and kept; the names are static, so a test module lists them without building any.
AHEAD = 3072            # gss_track.hip: samples of an epoch the fast form loads ahead
FIRST_FLUSH = 64512     # AHEAD + 30 passes of 2048: beyond it the int32 sums flush into int64
WSPAN = 2**31 // 1540 + 2
CS_MIN = M >> 23        # gss_trk_check: the code step stays above this, so an epoch is < 2^23

# (fs, epochs): the lengths 1..3, the wave and workgroup edges, one sample a chip, the end of the
# samples loaded ahead, the first lane that takes a second sample of a four-sample pass (3,584:
# below it only the pass's first sample is live, so its later masks and phase steps do not
# show), the end of the first pass, the first flush, and 130 MS/s
RATE_TABLE = ((1001, 40), (2046, 40), (63000, 12), (65000, 12), (511000, 12), (512000, 12),
              (513000, 12), (1023000, 12), (3071000, 10), (3072000, 10), (3073000, 10),
              (3584000, 10), (5120000, 8), (5121000, 8), (64512000, 6), (64513000, 6),
              (130000000, 5))
RATES = [f"rate_{fs}_sc{fmt:02d}" for fs, _ in RATE_TABLE for fmt in (16, 8, 1)]
SATURATING = ["saturating", "saturating_inverted"]
FEEDBACK_FS = (64000, 3073000)
FEEDBACK = [f"feedback_{fs}_{k}" for fs in FEEDBACK_FS
            for k in ("pull0", "pullall", "nogain", "wrap", "maxkd", "zeros", "negfull")]
ENDS_FS = (64000, 5121000)
ENDS = [f"ends_{fs}_{k}" for fs in ENDS_FS
        for k in ("exact", "short", "sc01_n0", "sc01_n1", "sc01_n2", "sc01_n3")]
LONGEST = "longest_epoch"


def kd_max(fs):
    """the largest Kd gss_trk_check admits at fs"""
    cn = cs_nominal(fs)
    return min(2**30, 4 * (cn - WSPAN - 2 - CS_MIN - 1) + 3, 4 * (M - cn - WSPAN - 2 - 1) + 3)


def chips_of(prn):
    """the +-1 chips of a PRN, int64 [1023]"""
    row = G.ca_table()[prn - 1]
    k = np.arange(1023)
    return 2 * ((row[k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(np.int64) - 1


def pack(xi, xq, fmt):
    """the bytes of samples (xI, xQ) in a format (SC01: +1 is a set bit, MSB first)"""
    v = np.empty(2 * len(xi), np.int64)
    v[0::2], v[1::2] = xi, xq
    if fmt == 16:
        return v.astype("<i2").view(np.uint8)
    if fmt == 8:
        return v.astype(np.int8).view(np.uint8)
    return np.packbits((v > 0).astype(np.uint8))


def lengths(c, j):
    """the lengths of job j's epochs but the last, from the records' first samples"""
    return np.diff(c["rec"]["s"][j, :c["count"][j]])


def _finish(fs, fmt, N, gains, jobs, data, pitch=None):
    pitch = pitch or max(max(j[3] for j in jobs), 1)
    rec, count = track(data, fmt, N, fs, gains, jobs, pitch)
    return dict(fs=fs, fmt=fmt, N=N, gains=gains, jobs=jobs, pitch=pitch, data=data, rec=rec,
                count=count)


def _rate(fs, ne, fmt):
    """three jobs as in shapes(): w0 of +1234 Hz, -2750 Hz and -2^31; the last starts so late
    that it runs out of samples inside an epoch; n_pull = 3 lies inside the run"""
    T = -(-fs // 1000)
    N = ne * fs // 1000 + T // 2 + 7
    jobs = [(1, 3, _w(1234, fs), ne), (17, T // 2 + 1, _w(-2750, fs), ne - ne // 4),
            (32, N - (3 * ne + 2) * fs // 6000, -2**31, ne)]
    return _finish(fs, fmt, N, gains_of(fs, 3), jobs, random_samples(N, fmt, fs % 9973 + fmt))


def _saturating(inverted):
    """Every product of the prompt correlator at its largest, all of one sign: xI = 32767 where
    cos * chip >= 0, else -32768, xQ likewise with sin.  With all gains 0 the phases are those
    of the start, so the samples can be written down; one lane of the kernel (every 512th sample
    of an epoch) sums past 2^31."""
    fs, prn = 130000000, 5
    w0 = _w(1234567, fs)
    cs = cs_nominal(fs) + tdiv(w0, 1540)
    N = -(-3 * M // cs) + 5
    i = np.arange(N, dtype=np.int64)
    p = chips_of(prn)[((i * cs) % M) >> 32]
    sin512, cos512 = (t.astype(np.int64) for t in G.lut())
    idx = ((i * w0) % 2**32) >> 23
    xi = np.where((cos512[idx] * p >= 0) != inverted, 32767, -32768)
    xq = np.where((sin512[idx] * p >= 0) != inverted, 32767, -32768)
    return _finish(fs, 16, N, (0, 0, 0, 0, 0), [(prn, 0, w0, 3)], pack(xi, xq, 16))


def lane_sums(c, lanes=512):
    """the prompt I sums of epoch 0 of job 0 as the fast form's lanes hold them: int64 [lanes]"""
    prn, s0, w0, _ = c["jobs"][0]
    n = int(lengths(c, 0)[0])
    cs = cs_nominal(c["fs"]) + tdiv(w0, 1540)
    xi, xq = unpack(c["data"], c["fmt"], c["N"])
    i = np.arange(n, dtype=np.int64)
    sin512, cos512 = (t.astype(np.int64) for t in G.lut())
    idx = ((i * w0) % 2**32) >> 23
    y = (xi[s0:s0 + n] * cos512[idx] + xq[s0:s0 + n] * sin512[idx]) * chips_of(prn)[(i * cs) >> 32]
    return np.bincount(i % lanes, weights=y.astype(np.float64)).astype(np.int64), np.abs(y).max()


def _feedback(fs, kind):
    """30 epochs of three jobs, w0 of -2^31, 2^31 - 1 and 900 Hz, with the loop at the ends of
    its arguments"""
    ne, T = 30, -(-fs // 1000)
    N = (ne + 8) * T                                     # maxkd: epochs up to a fifth longer
    d = defaults(fs)
    gains = {"pull0": (0,) + d[1:], "pullall": (ne + 5,) + d[1:], "nogain": (7, 0, 0, 0, 0),
             "wrap": (15, 2**30, 2**30, 2**30, d[4]), "maxkd": (3,) + d[1:4] + (kd_max(fs),),
             "zeros": (3,) + d[1:], "negfull": (3,) + d[1:]}[kind]
    jobs = [(2, 1, -2**31, ne), (11, T // 3, 2**31 - 1, ne), (30, 5, _w(900, fs), ne)]
    if kind == "zeros":
        data = np.zeros(4 * N, np.uint8)
    elif kind == "negfull":
        data = np.full(2 * N, -32768, "<i2").view(np.uint8)
    else:
        data = random_samples(N, 16, fs % 9973 + len(kind))
    return _finish(fs, 16, N, gains, jobs, data)


def _ends_jobs(fs, N, w):
    """behind job 0 (40 epochs from sample 5): starts at the last sample, at N and far behind it
    (count 0), n_epoch 0 and 1, and a job that runs out of samples in its eleventh epoch"""
    return [(3, 5, w, 40), (7, N - 1, w, 5), (8, N, -w, 5), (9, N + 10**6, w, 5), (12, 7, w, 0),
            (13, 11, -w, 1), (21, N - 21 * fs // 2000, w, 40)]


def _ends(fs, kind):
    """N from the oracle, so that job 0's last epoch ends exactly at N ("exact": 40 epochs) or
    one sample behind it (39); SC01 with four jobs of every s0 % 4 and N - 0..3 of every N % 4.
    The pitch is larger than every n_epoch."""
    fmt = 1 if kind.startswith("sc01") else 16
    key = ("ends", fs, fmt)
    w = _w(700, fs)
    first = [(3, 5, w, 41)] if fmt == 16 else [(3, 4, w, 41)]
    if key not in _want:
        N0 = 42 * -(-fs // 1000) + 16
        data = random_samples(N0, fmt, fs % 9973 + 50 + fmt)
        rec, count = track(data, fmt, N0, fs, gains_of(fs, 3), first, 41)
        assert count[0] == 41
        _want[key] = (data, int(rec["s"][0, 40]))
    data, N = _want[key]
    if fmt == 16:
        N -= kind == "short"
        jobs = _ends_jobs(fs, N, w)
    else:
        N -= int(kind[-1])
        jobs = [(3 + 5 * k, 4 + k, w if k % 2 == 0 else -w, 40) for k in range(4)]
    nb = 4 * N if fmt == 16 else (N + 3) // 4
    return _finish(fs, fmt, N, gains_of(fs, 3), jobs, data[:nb].copy(), pitch=64)


def longest_cfg():
    """(fs, gains) with cs_nom - span one above the bound of gss_trk_check, and the same one
    step of Kd / 4 further, which the calls reject"""
    fs = 2000000000
    kd = kd_max(fs)
    assert cs_nominal(fs) - (WSPAN + kd // 4 + 2) == CS_MIN + 1
    return fs, (0, 0, 0, 0, kd), (0, 0, 0, 0, kd + 1)


def _longest():
    """The longest epoch the limits admit, on SC01: 2 GS/s, w0 = -2^31 and the largest Kd.  Both
    bits of a sample are the late chip times the carrier's sign (w0 is half a cycle a sample), so
    the late envelope is full, the early one nearly empty, D_dll close to -2^14 and the second
    epoch's code step close to its floor."""
    fs, gains, _ = longest_cfg()
    cs = cs_nominal(fs) + tdiv(-2**31, 1540)
    N = -(-M // cs) + (1 << 23)
    i = np.arange(N, dtype=np.int64)
    x = chips_of(1)[(((i * cs) - HALF) % M) >> 32] * (1 - 2 * (i & 1))
    return _finish(fs, 1, N, gains, [(1, 0, -2**31, 2)], pack(x, x, 1))


def case(name):
    if name not in _want:
        kind, _, rest = name.partition("_")
        if kind == "rate":
            fs, fmt = rest.split("_sc")
            _want[name] = _rate(int(fs), dict(RATE_TABLE)[int(fs)], int(fmt))
        elif kind == "saturating":
            _want[name] = _saturating(rest == "inverted")
        elif kind == "feedback":
            fs, k = rest.split("_")
            _want[name] = _feedback(int(fs), k)
        elif kind == "ends":
            fs, k = rest.split("_", 1)
            _want[name] = _ends(int(fs), k)
        else:
            assert name == LONGEST
            _want[name] = _longest()
    return _want[name]


# ---- the physical test's inputs --------------------------------------------------------------
# The first 12.5 s (125 blocks) of the static scenario at 1 MS/s (asked for 12.6 s: the block
# count of a duration rounds down, and 12.5 gives 124), rendered by the CPU oracle from
# Scenario.next rows, with noise as acq_oracle.noisy_block adds it (PHYS_CN0, seed 7).  The
# search over block 0 uses 250 Hz bins: the frequency-locked pull-in reaches +-125 Hz.
PHYS_BLOCKS = 125
PHYS_DURATION = 12.6
PHYS_EPOCHS = 12400
PHYS_DF, PHYS_K, PHYS_M = 250, 20, 10
# Tracked C/N0 minus the request corrected by the row's gain [dB].  Measured on this scenario
# (eleven satellites, noise for 50 dB-Hz at full gain, seed 7): SC16 -1.48..-0.99, SC08
# -1.49..-1.00, SC01 -3.38..-2.87 (not asserted).  The one-satellite prototype read -0.15: the
# rest is the other ten satellites' cross-correlation, which alone (no noise) puts a floor 4.1 to
# 6.3 dB under each signal's request; 1 / (10^-4.914 + 10^-5.549) is 48.2 dB-Hz for PRN 17, the
# -0.99.  The bound is the measured range plus 0.5 dB, inside check_physical's 3 dB.
LEVEL = (-2.0, -0.5)
_phys = {}


def phys_rows():
    """(blk [125, 16], nch [125], nav table, n_per_blk) of the run"""
    from conftest import LOC, NAV
    import acq_oracle as A
    if "rows" not in _phys:
        s = G.Scenario(NAV, llh=LOC, duration=PHYS_DURATION, samp_freq=float(A.PHYS_FS))
        blk, nch = s.next(PHYS_BLOCKS)
        assert len(nch) == PHYS_BLOCKS
        _phys["rows"] = (blk, nch, s.nav_table().copy(), s.n_per_blk)
        s.close()
    return _phys["rows"]


def phys_iq():
    """the run's noise-free samples as int16, rendered by the CPU oracle"""
    import oracle
    if "iq" not in _phys:
        blk, nch, nav, n_per_blk = phys_rows()
        out, rc = oracle.synth(blk, nch, G.ca_table(), nav, n_per_blk, 16)
        assert rc == 0
        _phys["iq"] = out.view(np.int16).copy()
    return _phys["iq"]


def phys_sigma():
    import acq_oracle as A
    return int(np.floor(256 * 250 * np.sqrt(A.PHYS_FS / (2 * 10 ** (A.PHYS_CN0 / 10))) + 0.5))


def phys_samples(fmt, clean=False):
    import acq_oracle as A
    key = (fmt, clean)
    if key not in _phys:
        iq = phys_iq()
        sigma = 0 if clean else phys_sigma()
        shift = 2 if (fmt == 8 and not clean) else 0
        _phys[key] = G.impair_host(G.Impair(sigma, shift, 7), iq, 0, fmt)
    return _phys[key]


def phys_acq(fmt):
    import acq_oracle as A
    return G.Acq(A.PHYS_FS, fmt, 1, PHYS_M, PHYS_DF, PHYS_K, -1)


def steady_channels(blk, nch):
    """{prn: slot} of the channels that stay allocated, in one slot, over every block"""
    first = {int(r["ca_tbl"]) + 1: k for k, r in enumerate(blk[0][:nch[0]])}
    keep = {}
    for prn, k in first.items():
        if all(k < nch[b] and int(blk[b][k]["ca_tbl"]) + 1 == prn for b in range(len(nch))):
            keep[prn] = k
    return keep


def phys_jobs(fmt, peaks):
    """jobs for the PRNs of the steady channels from the search's peaks"""
    blk, nch = phys_rows()[:2]
    keep = steady_channels(blk, nch)
    sel = np.array([p for p in peaks if int(p["prn"]) in keep], G.ACQ_PEAK_DTYPE)
    return G.trk_jobs(phys_acq(fmt), sel, 0, PHYS_EPOCHS), keep


def check_decode(rec, count, jobs, keep, level=None, want_sf=1, every_bit=False):
    """Every steady PRN yields >= want_sf subframes; each equals ten words [10 k, 10 k + 10) of
    its channel's nav row, and begins, within acquisition's E samples, where the row's code
    phase advanced from its block start says word 10 k, bit 0, code period 0 begins.  level: a
    (lo, hi) bound on tracked C/N0 minus the request corrected by the row's gain.  every_bit:
    every subframe whose 300 bits lie behind the bit synchronisation's start was decoded."""
    import acq_oracle as A
    blk, nch, nav, n_per_blk = phys_rows()
    E = A.PHYS_ACQ(16).sizes()[3]
    out = {}
    for j, job in enumerate(jobs):
        prn, k = int(job["prn"]), keep[int(job["prn"])]
        r = rec[j, :count[j]]
        assert count[j] == PHYS_EPOCHS, (prn, count[j])
        sfs, off = G.nav_decode(r)
        print("PRN", prn, "subframes", len(sfs), "bit offset", off, "cn0", G.trk_cn0(r),
              "doppler", float(r[-1]["w"]) * A.PHYS_FS / 2**32)
        assert len(sfs) >= want_sf, (prn, len(sfs))
        for sf in sfs:
            b, i = divmod(int(sf["sample"]), n_per_blk)
            row = blk[b][k]
            words = nav[row["nav_tbl"]]
            hit = [q for q in range(6) if np.array_equal(words[10 * q:10 * q + 10], sf["word"])]
            assert hit, (prn, sf)
            ok = False
            for d in range(-E, E + 1):
                bb, ii = divmod(int(sf["sample"]) + d, n_per_blk)
                rw = blk[bb][k]
                ph, ic, ib, iw = G.code_advance(rw["code0"], rw["code_step"], ii, rw["icode"],
                                                rw["ibit"], rw["iword"])
                if ph < rw["code_step"] and ic == 0 and ib == 0 and iw % 10 == 0 and np.array_equal(
                        nav[rw["nav_tbl"]][iw:iw + 10], sf["word"]):
                    ok = True
            assert ok, (prn, sf)
        if every_bit:
            # subframes last 6000 epochs: all that fit behind epoch 500 + 19 must be there
            first = int(sfs[0]["epoch"])
            assert first < 500 + 20 + 40 + 6000, (prn, first)
            for a, b in zip(sfs[:-1], sfs[1:]):
                assert int(b["epoch"]) - int(a["epoch"]) == 6000, (prn, a, b)
            assert PHYS_EPOCHS - int(sfs[-1]["epoch"]) < 2 * 6000 + 20, (prn, sfs[-1])
        if level is not None:
            t = G.acq_expect(blk[0][k], A.PHYS_FS, 0)
            diff = G.trk_cn0(r) - (A.PHYS_CN0 + t["cn0_offset_db"])
            print("   level", G.trk_cn0(r), A.PHYS_CN0 + t["cn0_offset_db"], diff)
            assert level[0] <= diff <= level[1], (prn, diff)
        out[prn] = sfs
    assert set(out) == set(keep)
    return out
