"""The fast kernel's chunk records (csrc/common/gss_lin.h: gss_lin_chunk_rec) on the CPU.

A wave of gss_lin_kernel renders its 4096-sample segment in four chunks of 1024 samples and makes
the four chunks' parameters of every channel in one pass, lane 16 c + k for chunk c of channel k:
the anchor base B, the byte offsets wa / wn of the chunk's and the next chunk's window-table rows,
the flags (gain change inside the chunk, patched samples) and the signed gain at the chunk's first
sample.  The same function compiles with gcc (tests/helpers/lin_chunk_rec.c); here it is compared
with a restatement in Python integers (exact, any size) for c = 0..3:

* the rows of random certified lines (synth_params through gss_linearize) at every segment start;
* the code base chip on, below and above the last row of the window table (the clamp at
  GSS_LIN_TWE - 1), for the chunk's row and for the next chunk's alone;
* the first gain change (pos1) on a chunk's first sample, its last sample and the sample after
  its last, for every chunk, and pos1 = INT32_MAX; patch counts of 0, 1 and many;
* code steps at both ends of the range gss_lin_win16_ok certifies at 2.6 MS/s;
* the next chunk's row of chunk c is the row of chunk c + 1 (the kernel takes it from there).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from test_lin_rows import blank_line, c_chan, c_row
from test_linearize import synth_params

import gpssim_amd as G

HELP = os.path.join(REPO, "tests", "helpers")
SEG, CHUNK, CH, TWE = 4096, 1024, 16, 2560
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
I32MAX = (1 << 31) - 1
U50 = 1 << 50
GAIN, PATCH = 1, 2
_lc = None


def lc():
    global _lc
    if _lc is None:
        src = os.path.join(HELP, "lin_chunk_rec.c")
        so = os.path.join(HELP, "_lin_chunk_rec.so")
        hdr = os.path.join(PKG, "csrc", "common", "gss_lin.h")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src),
                                                                 os.path.getmtime(hdr)):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.lc_rec.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
        L.lc_win16_ok.argtypes = [C.c_uint64, C.c_int]
        _lc = L
    return _lc


def c_rec(row, chan, n0, c):
    """(B, wa, wn, flags, g) of gss_lin_chunk_rec; row = (x, z, g01, pos1, npatch), chan = (xs,
    zs, tab)"""
    r = np.array([row[0], row[1], row[2] & M32, row[3] & M32, row[4]], np.uint64)
    ch = np.array(chan, np.uint64)
    out = np.zeros(6, np.int64)
    lc().lc_rec(r.ctypes.data, ch.ctypes.data, n0, c, out.ctypes.data)
    assert out[5] == 24
    return int(out[0]) & M64, int(out[1]), int(out[2]), int(out[3]), int(out[4])


# ---- the restatement: Python integers, 64-bit wrapping written out where the C wraps ----------
def py_wrow(tab, zb):
    return ((tab * TWE + min(zb >> 50, TWE - 1)) * (CH * 4)) & M32


def py_rec(row, chan, n0, c):
    x, z, g01, pos1, npatch = row
    xs, zs, tab = chan
    xb = (x + c * CHUNK * xs) & M64
    zb = (z + c * CHUNK * zs) & M64
    B = (xb & (M64 ^ M32)) | ((zb >> 26) & M32)
    nb0 = n0 + c * CHUNK
    after = pos1 <= nb0
    inside = nb0 < pos1 < nb0 + CHUNK
    g0, g1 = ((g01 & 0xFFFF) ^ 0x8000) - 0x8000, g01 >> 16
    return (B, py_wrow(tab, zb), py_wrow(tab, (zb + CHUNK * zs) & M64),
            (GAIN if inside else 0) | (PATCH if npatch else 0), g1 if after else g0)


def check(row, chan, n0, tag):
    recs = [c_rec(row, chan, n0, c) for c in range(SEG // CHUNK)]
    for c, r in enumerate(recs):
        assert r == py_rec(row, chan, n0, c), (tag, c)
    for c in range(SEG // CHUNK - 1):
        assert recs[c][2] == recs[c + 1][1], (tag, c)            # wn of c = wa of c + 1
    return recs


def g01_of(g0, g1):
    v = (g0 & 0xFFFF) | ((g1 & 0xFFFF) << 16)
    return v - (1 << 32) if v >> 31 else v


def zs_ends(n):
    """the least and the greatest code step (2^-50 chip per sample) gss_lin_win16_ok certifies for
    blocks of n samples at 10 n samples per second"""
    ok = lambda zs: bool(lc().lc_win16_ok(zs, n))               # noqa: E731
    mid = int(1.023e6 / (10.0 * n) * U50)
    assert ok(mid)
    lo, hi = 1, mid                                             # ok is an interval around mid
    while lo < hi:
        m = (lo + hi) // 2
        lo, hi = (lo, m) if ok(m) else (m + 1, hi)
    least = lo
    lo, hi = mid, U50
    while lo < hi:
        m = (lo + hi + 1) // 2
        lo, hi = (m, hi) if ok(m) else (lo, m - 1)
    assert ok(least) and not ok(least - 1) and ok(lo) and not ok(lo + 1)
    return least, lo


def test_records_of_certified_lines():
    """every (channel, segment) of random certified blocks, all four chunks"""
    rng = np.random.default_rng(77)
    n = 260000
    nchv = [12, 1, 16]
    blk, nch, nav = synth_params(rng, len(nchv), nchv, n)
    lin, fast = G.linearize(blk, nch, nav, n)
    assert fast.sum() >= 2, fast
    nrec, changes = 0, set()
    for b in np.nonzero(fast)[0]:
        for k in range(nch[b]):
            tab = int(blk[b, k]["ca_tbl"])
            ch = c_chan(lin[b, k], tab)
            for n0 in range(0, n, SEG):
                row = c_row(lin[b, k], n0)[:5]
                recs = check(row, (ch[0], ch[1], tab), n0, (int(b), k, n0))
                changes.update(c for c, r in enumerate(recs) if r[3] & GAIN)
                nrec += len(recs)
    assert nrec >= 13 * 64 * 4
    assert changes == {0, 1, 2, 3}          # the lines' gain changes reach every chunk position


@pytest.mark.parametrize("chip", [TWE - 2, TWE - 1, TWE, TWE + 440])
def test_window_row_clamp(chip):
    """the code base chip at the table's last row and past it: wa and wn stop at row TWE - 1 of
    the channel's C/A row; just below it only the next chunk's row is clamped"""
    rng = np.random.default_rng(chip)
    line = blank_line(rng)
    xs, zs = int(line["xs"]), int(line["zs"])
    for tab in (0, 31):
        for frac in (0, U50 - 1):
            row = (int(line["x0"]), (chip << 50) | frac, g01_of(50, 50), I32MAX, 0)
            recs = check(row, (xs, zs, tab), 8 * SEG, ("clamp", chip, tab, frac))
            last = (tab * TWE + TWE - 1) * 64
            if chip >= TWE - 1:
                assert all(r[1] == last and r[2] == last for r in recs)
            else:
                assert recs[0][1] == (tab * TWE + chip) * 64 and recs[0][2] == last


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_gain_change_on_chunk_edges(c):
    rng = np.random.default_rng(40 + c)
    line = blank_line(rng)
    chan = (int(line["xs"]), int(line["zs"]), 7)
    n0 = 5 * SEG
    first = n0 + c * CHUNK
    x, z = int(line["x0"]), (700 << 50) | 12345
    for npatch in (0, 1, 9):
        pf = PATCH if npatch else 0
        # (pos1, flags of chunk c, gain of chunk c, gain of the chunk after)
        for pos1, fl, g, g_next in [(first, pf, -88, -88),              # changed before sample 0
                                    (first + CHUNK - 1, pf | GAIN, 88, -88),
                                    (first + CHUNK, pf, 88, -88),        # the next chunk's first
                                    (first + 1, pf | GAIN, 88, -88),
                                    (I32MAX, pf, 88, 88)]:
            if pos1 != I32MAX and pos1 >= n0 + SEG:
                continue                                 # (a row's pos1 lies inside its segment)
            row = (x, z, g01_of(88, -88), pos1, npatch)
            recs = check(row, chan, n0, ("edge", c, pos1, npatch))
            assert (recs[c][3], recs[c][4]) == (fl, g)
            assert all(r[4] == 88 and r[3] == pf for r in recs[:c])
            if c < 3:
                assert recs[c + 1][4] == g_next
                # a change on the next chunk's first sample is no change inside either chunk
                assert recs[c + 1][3] == pf


def test_code_step_at_the_ends_of_the_certified_range():
    n = 260000
    least, most = zs_ends(n)
    assert least < int(1.023e6 / 2.6e6 * U50) < most
    assert 63 * most + 3 * U50 <= 31 * U50                         # GSS_LIN_WIN_OK holds too
    rng = np.random.default_rng(9)
    for zs in (least, most):
        for e0 in (1, 512, 1023):
            for xs in (0, 1, M64, int(rng.integers(0, 1 << 63))):
                row = (int(rng.integers(0, 1 << 63)) * 2 + 1, (e0 << 50) | int(rng.integers(U50)),
                       g01_of(-1024, 1024), 3 * SEG + 2 * CHUNK + 5, 0)
                recs = check(row, (xs, zs, 31), 3 * SEG, ("zs", zs, e0, xs))
                assert [r[3] for r in recs] == [0, 0, GAIN, 0]
                assert [r[4] for r in recs] == [-1024, -1024, -1024, 1024]
                # a certified channel stays inside the table: no clamp
                assert all(r[1] < (31 * TWE + TWE - 1) * 64 for r in recs)
