"""The front-end filter's definition (include/gpssim_amd.h, gss_fir_t) restated with numpy int64,
independent of csrc/common/gss_fir.h: what gss_fir_host and the kernels are compared with.  Every
call of fir() checks itself against plain Python integers on a few hundred samples."""
import math

import numpy as np

MAXTAP = 64
L1_MAX = 65535


def quantise(v, fmt):
    """The output stage on int64 values v (I, Q interleaved): the bytes of format fmt as uint8."""
    v = np.asarray(v, np.int64)
    if fmt == 16:
        return np.clip(v, -32768, 32767).astype("<i2").view(np.uint8)
    if fmt == 8:
        return np.clip(v >> 4, -128, 127).astype(np.int8).view(np.uint8)
    assert fmt == 1 and v.size % 8 == 0
    return np.packbits((v > 0).astype(np.uint8))           # MSB first, the reference's order


def values(taps, iq, halo=None):
    """v = (acc + 2^13) >> 14 for every component of iq (int16[2 n], I and Q interleaved); halo:
    the len(taps) - 1 samples before them (int16[2 (T - 1)]) or None for zeros."""
    taps = np.asarray(taps, np.int64)
    T = len(taps)
    x = np.asarray(iq, np.int64).reshape(-1, 2)
    n = len(x)
    pre = np.zeros((T - 1, 2), np.int64)
    if halo is not None:
        pre[:] = np.asarray(halo, np.int64).reshape(T - 1, 2)
    ext = np.concatenate([pre, x])                          # ext[T - 1 + i] = x[i]
    acc = np.zeros((n, 2), np.int64)
    for c in (0, 1):                    # valid[i] = sum_k taps[k] * ext[i + T - 1 - k], in int64
        if n:
            acc[:, c] = np.convolve(np.ascontiguousarray(ext[:, c]), taps, mode="valid")
    assert n == 0 or np.abs(acc).max() < 2 ** 31
    v = (acc + 8192) >> 14
    # the same from Python integers, on the first and last samples
    ext_l = ext.tolist()
    tl = [int(t) for t in taps]
    for i in sorted(set(list(range(min(n, 150))) + list(range(max(0, n - 150), n)))):
        for c in (0, 1):
            a = sum(tl[k] * ext_l[T - 1 + i - k][c] for k in range(T))
            assert (a + 8192) >> 14 == int(v[i, c]), (i, c)
    return v.reshape(-1)


def fir(taps, iq, halo, fmt):
    """The filter's bytes of format fmt (uint8)."""
    return quantise(values(taps, iq, halo), fmt)


def check(n_taps, pad, taps):
    """True when gss_fir_check accepts the filter."""
    return 1 <= n_taps <= MAXTAP and pad == 0 and sum(abs(int(t)) for t in taps[:n_taps]) <= L1_MAX


def make(fs_hz, bw_hz, n_taps):
    """gss_fir_make's formula in numpy doubles: the taps as a list of ints."""
    M = n_taps - 1
    c = bw_hz / fs_hz
    k = np.arange(n_taps)
    m = k - M // 2
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m == 0, c, np.sin(np.pi * c * m) / (np.pi * m))
    d = s * (0.54 - 0.46 * np.cos(2 * np.pi * k / M))
    S = 0.0
    for v in d:
        S += float(v)
    t = np.floor(d / S * 16384 + 0.5).astype(np.int64)
    t[M // 2] += 16384 - t.sum()
    return [int(v) for v in t]


def response_db(taps, f_over_fs):
    """|H(f)| in dB at the normalised frequencies f_over_fs, gain 1 = 16384"""
    taps = np.asarray(taps, np.float64) / 16384.0
    k = np.arange(len(taps))
    f = np.atleast_1d(np.asarray(f_over_fs, np.float64))
    H = np.exp(-2j * np.pi * np.outer(f, k)) @ taps
    return 20 * np.log10(np.maximum(np.abs(H), 1e-12))


def noise_gain(taps):
    return sum(int(t) * int(t) for t in taps) / 2.0 ** 28


def extreme_taps(T, sign):
    """T taps with sum |h| = 65535 (T = 1: the largest an int16 holds), all positive (sign 1), all
    negative (-1) or alternating (0)"""
    if T == 1:
        return [32767 if sign == 1 else -32768]
    base, rem = divmod(L1_MAX, T)
    mag = [base + (1 if k < rem else 0) for k in range(T)]
    sg = [sign if sign else (1 if k % 2 == 0 else -1) for k in range(T)]
    if T == 2 and sign == 1:                                 # 32768 has no positive int16
        mag = [32767, 32767]
    t = [-m if m == 32768 else s * m for m, s in zip(mag, sg)]
    assert all(-32768 <= v <= 32767 for v in t) and sum(abs(v) for v in t) <= L1_MAX
    return t


def sign_matched(taps, n, at, level=32767):
    """int16[2 n] input whose sample at - k is level * sign(taps[k]): acc at `at` is level * sum |h|"""
    x = np.zeros((n, 2), np.int16)
    for k, h in enumerate(taps):
        if 0 <= at - k < n:
            x[at - k] = level if h >= 0 else -level
    return x.reshape(-1)


def random_taps(rng, T):
    """random taps of both signs with sum |h| <= 65535"""
    t = rng.integers(-32768, 32768, T)
    while np.abs(t).sum() > L1_MAX:
        t = t // 2
    return [int(v) for v in t]


def group_delay(n_taps):
    return (n_taps - 1) // 2


assert math.isclose(noise_gain([16384]), 1.0)
