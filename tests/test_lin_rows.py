"""The fast kernel's segment rows (csrc/common/gss_lin.h: gss_lin_row_at, gss_lin_chan_of) on the
CPU.

gss_lin_kernel builds, per workgroup and in its set-up, the rows its waves start from: per
(channel, 4096-sample wave segment) the carrier and code anchor bases, the gain pair with the
sample of the first gain change, and the patch count; per channel the step constants.  The same
functions compile with gcc (tests/helpers/lin_rows.c); here they are compared with a restatement
in Python integers (exact, any size):

* random certified lines (synth_params through gss_linearize) at every segment start of a block;
* constructed lines: a chip count at a segment start that is an exact multiple of 1023 (reduced
  to 1023, not 0), a 64-bit code sum that wraps past z0 (the carry into the high word), a gain
  change exactly on a segment start and on its last sample, patches on a segment's first and last
  sample;
* for a sample of positions p, the LUT cell and chip that follow from the row by chunk and step
  advances (the kernel's walk) equal gss_lin_kernel_at(p), the model the proof certifies.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from test_linearize import synth_params

import gpssim_amd as G

HELP = os.path.join(REPO, "tests", "helpers")
SEG, CHUNK, CH = 4096, 1024, 16
M64 = (1 << 64) - 1
I32MAX = (1 << 31) - 1
_lr = None


def lr():
    global _lr
    if _lr is None:
        src = os.path.join(HELP, "lin_rows.c")
        so = os.path.join(HELP, "_lin_rows.so")
        hdrs = [os.path.join(REPO, "include", "gpssim_amd.h"),
                os.path.join(PKG, "csrc", "common", "gss_lin.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(
                [os.path.getmtime(src)] + [os.path.getmtime(h) for h in hdrs]):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.lr_row.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.lr_chan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.lr_kernel_at.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.lr_lane.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.lr_lane.restype = C.c_uint64
        L.lr_sizes.argtypes = [C.c_int]
        _lr = L
    return _lr


def c_row(line, n0):
    """(x, z, g01, pos1, npatch, pad) of gss_lin_row_at"""
    one = np.ascontiguousarray(line).reshape(1)
    out = np.zeros(6, np.int64)
    lr().lr_row(one.ctypes.data, n0, out.ctypes.data)
    return (int(out[0]) & M64, int(out[1]) & M64, int(out[2]), int(out[3]), int(out[4]),
            int(out[5]))


def c_chan(line, tab):
    one = np.ascontiguousarray(line).reshape(1)
    out = np.zeros(5, np.uint64)
    lr().lr_chan(one.ctypes.data, tab, out.ctypes.data)
    return tuple(int(v) for v in out)


def c_kernel_at(line, p):
    one = np.ascontiguousarray(line).reshape(1)
    out = np.zeros(2, np.int32)
    lr().lr_kernel_at(one.ctypes.data, p, out.ctypes.data)
    return int(out[0]), int(out[1])


# ---- the restatement: Python integers, 64-bit wrapping written out where the C wraps ----------
def s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def tdiv2(v):
    """C's v / 2 (towards zero)"""
    return -((-v) // 2) if v < 0 else v // 2


def py_dx(xs):
    return ((((xs * 64) & M64) + (1 << 31)) & M64) >> 32


def py_dz(zs):
    return (((((zs * 64) & M64) + (1 << 25)) & M64) >> 26) & 0xFFFFFFFF


def py_xa(xs):
    e = s64((py_dx(xs) << 32) - xs * 64)
    return ((1 << 31) - tdiv2(e * (CH - 1))) & M64


def py_za(zs):
    ec = s64((py_dz(zs) << 26) - zs * 64)
    return ((1 << 25) - tdiv2(ec * (CH - 1))) & M64


def py_row(line, n0):
    x0, xs, z0, zs = (int(line[f]) for f in ("x0", "xs", "z0", "zs"))
    x = (x0 + n0 * xs + py_xa(xs)) & M64
    Z = z0 + n0 * zs                                   # the unwrapped code line, exact
    chips, frac = Z >> 50, Z & ((1 << 50) - 1)
    e0 = chips % 1023 or 1023
    z = (((e0 << 50) | frac) + py_za(zs)) & M64
    gpos, gval = [int(v) for v in line["gpos"]], [int(v) for v in line["gval"]]
    q = 0                                              # gpos ascending, gpos[0] = 0
    while q + 1 < len(gpos) and gpos[q + 1] <= n0:
        q += 1
    g0 = gval[q]
    more = q + 1 < len(gpos) and gpos[q + 1] < n0 + SEG
    g1 = gval[q + 1] if more else g0
    g01 = (g0 & 0xFFFF) | ((g1 << 16) & 0xFFFFFFFF)
    g01 = g01 - (1 << 32) if g01 >> 31 else g01
    pos1 = gpos[q + 1] if more else I32MAX
    npatch = sum(1 for v in line["ppos"] if n0 <= int(v) < n0 + SEG)
    return x, z, g01, pos1, npatch, 0


def py_chan(line, tab):
    xs, zs = int(line["xs"]), int(line["zs"])
    return xs, zs, (py_dx(xs) << 32) | py_dz(zs), ((zs * 64) & M64) >> 46, tab


def py_lane(xs, zs, l):
    lx = ((((l * xs) & M64) + (1 << 31)) & M64) >> 32
    lz = (((l * zs) & M64) >> 26) & 0xFFFFFFFF
    return (lx << 32) | lz


def walk_from_row(line, row, chan, p):
    """cell and chip at block sample p as gss_lin_kernel reaches them: the row's bases advanced by
    whole chunks, the lane offset added at the anchor, one 64-bit add of D per step"""
    n0 = p & ~(SEG - 1)
    ci, s, ln = (p - n0) // CHUNK, ((p - n0) % CHUNK) >> 6, p & 63
    xs, zs, D = chan[0], chan[1], chan[2]
    xb = (row[0] + ci * ((xs << 10) & M64)) & M64
    zb = (row[1] + ci * ((zs << 10) & M64)) & M64
    B = (xb & (M64 ^ 0xFFFFFFFF)) | ((zb >> 26) & 0xFFFFFFFF)
    lane = py_lane(xs, zs, ln)
    assert lane == lr().lr_lane(xs, zs, ln)
    P = (lane + B) & M64
    for _ in range(s):
        P = (P + D) & M64
    kz = (zb >> 26) + (lane & 0xFFFFFFFF) + s * (D & 0xFFFFFFFF)     # the code word, unwrapped
    assert kz & 0xFFFFFFFF == P & 0xFFFFFFFF
    return P >> 55, (kz >> 24) % 1023


def check_line(line, n, tab, rng, tag):
    assert c_chan(line, tab) == py_chan(line, tab), tag
    chan = c_chan(line, tab)
    for n0 in range(0, n, SEG):
        row = c_row(line, n0)
        assert row == py_row(line, n0), (tag, n0)
        last = min(n0 + SEG, n) - 1
        ps = {n0, last, min(n0 + CHUNK - 1, last), min(n0 + CHUNK, last),
              min(n0 + 3 * CHUNK + 64, last)}
        ps.update(int(v) for v in rng.integers(n0, last + 1, size=3))
        for p in sorted(ps):
            assert walk_from_row(line, row, chan, p) == c_kernel_at(line, p), (tag, p)


def blank_line(rng, gain=100):
    """a line with realistic steps (2.6 MS/s), one gain entry and no patches"""
    line = np.zeros((), G.LIN_DTYPE)
    f = float(rng.uniform(-5000, 5000))
    line["x0"] = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
    line["xs"] = int(round(f / 2.6e6 * 2.0 ** 64)) & M64
    line["z0"] = int(rng.random() * 1023 * 2.0 ** 50)
    line["zs"] = int((1.023e6 + f / 1540.0) / 2.6e6 * 2.0 ** 50)
    line["gpos"] = [0] + [I32MAX] * (G.NGC - 1)
    line["gval"] = [gain] + [0] * (G.NGC - 1)
    line["ppos"] = I32MAX
    return line


def test_struct_sizes():
    assert lr().lr_sizes(0) == 32 and lr().lr_sizes(1) == 32


def test_rows_of_certified_lines():
    """every (channel, segment) row of random certified blocks, all segments of the block"""
    rng = np.random.default_rng(2024)
    n = 260000
    nchv = [12, 1, 16]
    blk, nch, nav = synth_params(rng, len(nchv), nchv, n)
    lin, fast = G.linearize(blk, nch, nav, n)
    assert fast.sum() >= 2, fast
    nrows = 0
    for b in np.nonzero(fast)[0]:
        for k in range(nch[b]):
            check_line(lin[b, k], n, int(blk[b, k]["ca_tbl"]), rng, (int(b), k))
            nrows += 1
    assert nrows >= 13


@pytest.mark.parametrize("seg", [1, 7, 63])
def test_chip_count_multiple_of_1023(seg):
    """floor(Z(n0) / 2^50) an exact multiple of 1023 at a segment start: the reduced chip is 1023
    (gss_lin_e0), so the anchor offset cannot take the reduced line below zero"""
    rng = np.random.default_rng(seg)
    for frac in (0, 1, (1 << 50) - 1, int(rng.integers(0, 1 << 50))):
        line = blank_line(rng)
        zs, n0 = int(line["zs"]), seg * SEG
        m = -(-(n0 * zs) // (1023 << 50))                   # least m with 1023 m chips >= n0 zs
        line["z0"] = m * (1023 << 50) + frac - n0 * zs      # in [0, 1024 chips)
        assert ((int(line["z0"]) + n0 * zs) >> 50) % 1023 == 0
        row = c_row(line, n0)
        assert row == py_row(line, n0)
        assert (row[1] - py_za(zs)) & M64 == (1023 << 50) | frac
        check_line(line, (seg + 2) * SEG, 5, rng, ("e0", seg, frac))


def test_code_sum_wraps_past_z0():
    """z0 + (n0 zs mod 2^64) overflows 64 bits: the carry belongs to the high word of Z(n0)"""
    rng = np.random.default_rng(3)
    hit = 0
    for i in range(40):
        line = blank_line(rng)
        line["z0"] = M64 - int(rng.integers(0, 1 << 40))
        n = 20 * SEG
        zs = int(line["zs"])
        hit += sum(1 for n0 in range(0, n, SEG)
                   if ((n0 * zs) & M64) + int(line["z0"]) > M64)
        check_line(line, n, 31, rng, ("wrap", i))
    assert hit > 100


@pytest.mark.parametrize("at", ["start", "last", "next_start", "before_start"])
def test_gain_change_on_segment_edges(at):
    rng = np.random.default_rng(5)
    line = blank_line(rng, gain=77)
    n0 = 3 * SEG
    pos = {"start": n0, "last": n0 + SEG - 1, "next_start": n0 + SEG, "before_start": n0 - 1}[at]
    line["gpos"] = [0, pos, pos + 20 * SEG] + [I32MAX] * (G.NGC - 3)
    line["gval"] = [77, -77, 77] + [0] * (G.NGC - 3)
    row = c_row(line, n0)
    assert row == py_row(line, n0)
    g0, g1 = ((row[2] & 0xFFFF) ^ 0x8000) - 0x8000, row[2] >> 16
    want = {"start": (-77, -77, I32MAX),                    # already changed: no change inside
            "last": (77, -77, pos),
            "next_start": (77, 77, I32MAX),
            "before_start": (-77, -77, I32MAX)}[at]
    assert (int(g0), int(g1), row[3]) == want
    check_line(line, 8 * SEG, 0, rng, ("gain", at))


def test_patches_on_segment_edges():
    rng = np.random.default_rng(6)
    line = blank_line(rng)
    n0 = 2 * SEG
    line["ppos"] = [n0 - 1, n0, n0 + 5, n0 + SEG - 1, n0 + SEG, 5 * SEG - 1] + \
        [I32MAX] * (G.NPATCH - 6)
    counts = [c_row(line, s * SEG)[4] for s in range(6)]
    assert counts == [0, 1, 3, 1, 1, 0]
    check_line(line, 6 * SEG, 9, rng, "patch")
