"""numpy restatement of the additive-noise definition (include/gpssim_amd.h, gss_impair_t),
independent of the library: Philox4x32-10 words keyed on the absolute sample index, a
half-normal inverse-CDF table built here from statistics.NormalDist, the integer noise and the
three output formats.  Shared by tests/test_impair.py and tests/test_gpu_impair.py."""
import statistics

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key):
    """Philox4x32-10: ctr uint32[..., 4], key uint32[..., 2] (broadcast) -> uint32[..., 4]"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0 = np.asarray(key)[..., 0].astype(np.uint64)
    k1 = np.asarray(key)[..., 1].astype(np.uint64)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1,
             p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def check_known_answers():
    for ctr, key, want in KAT:
        got = philox4x32(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert tuple(int(v) for v in got) == want, (ctr, key, [hex(int(v)) for v in got])


_table = None


def table():
    """T[4097] int64, Q16: round(65536 Phi^-1(0.5 + i/8192)), the end at 1 - 1/32768"""
    global _table
    if _table is None:
        nd = statistics.NormalDist()
        ps = [0.5 + i / 8192 for i in range(4096)] + [1 - 1 / 32768]
        _table = np.array([int(np.floor(65536 * nd.inv_cdf(p) + 0.5)) for p in ps], np.int64)
    return _table


def words(seed, sample0, n):
    """uint32[n, 2]: the I and Q words of samples sample0 .. sample0 + n - 1"""
    check_known_answers()
    idx = np.arange(n, dtype=np.uint64) + np.uint64(sample0)
    c = idx >> np.uint64(1)
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = (c & MASK).astype(np.uint32)
    ctr[:, 1] = (c >> np.uint64(32)).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    w = philox4x32(ctr, key)
    odd = (idx & np.uint64(1)).astype(bool)
    return np.where(odd[:, None], w[:, 2:4], w[:, 0:2])


def noise(seed, sigma_q8, sample0, n):
    """int64[n, 2]: g of every component"""
    u = words(seed, sample0, n).astype(np.int64)
    T = table()
    idx, f = (u >> 19) & 4095, (u >> 3) & 0xFFFF
    mag = T[idx] + (((T[idx + 1] - T[idx]) * f) >> 16)
    g = (mag * int(sigma_q8) + (1 << 23)) >> 24
    return np.where((u >> 31) != 0, -g, g)


def impair(seed, sigma_q8, shift, iq, sample0, fmt, g=None):
    """the bytes (uint8) of format fmt for noise-free iq int16[2 n] from sample0 on (g: their
    noise(seed, sigma_q8, sample0, n), when the caller has it already)"""
    x = np.asarray(iq, np.int16).reshape(-1, 2).astype(np.int64)
    n = len(x)
    v = x + (noise(seed, sigma_q8, sample0, n) if g is None else g)
    w = (v + ((1 << shift) >> 1)) >> shift
    if fmt == 16:
        return np.clip(w, -32768, 32767).astype(np.int16).reshape(-1).view(np.uint8)
    if fmt == 8:
        return np.clip(w >> 4, -128, 127).astype(np.int8).reshape(-1).view(np.uint8)
    assert fmt == 1 and n % 4 == 0
    return np.packbits((w > 0).astype(np.uint8).reshape(-1))     # MSB first, gpssim.c:2273


# ---- the grid both test files run (the issue's cases) ------------------------------------------
SIGMAS = [0, 77, 256 * 994, 256 * 20000]          # the last two make every clamp fire
SHIFTS = [0, 3, 8]
STARTS = [0, 1, 2**32 - 5, 2**33 + 3]
SIZES = {16: [1, 7, 7803], 8: [1, 7, 7803], 1: [4, 8, 7804]}


def samples(n, seed=0):
    """int16[2 n] in the reference's range, with both extremes of int16 among them"""
    rng = np.random.default_rng(seed)
    iq = rng.integers(-2047, 2048, size=2 * n).astype(np.int16)
    iq[0], iq[-1] = -32768, 32767
    if n > 4:
        iq[5], iq[6] = 32767, -32768
    return iq
