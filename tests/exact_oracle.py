"""Inputs and harness for the exact render path (gss_anchor_kernel + gss_synth_kernel<NCH, FMT>,
csrc/hip/gss_synth.hip) against the scalar oracle of the reference loop.

rows() builds channel rows whose steps do not depend on the block length, SPECS names the row
sets the tests use (tests/test_exact_inputs.py checks every one of them on the CPU before
tests/test_gpu_exact.py hands it to a kernel), checkpoints() makes the carrier checkpoints by
brute force, on_device() runs one call between guard bytes and check() compares it with the
oracle.  Importing this module needs no GPU (torch is imported inside on_device only).
"""
import functools
import math

import numpy as np

import gpssim_amd as G
import oracle

E_RANGE = -8                      # GSS_E_RANGE
GUARD = 0xA5
U53 = 2.0 ** -53

# ---- step and start-value families -------------------------------------------------------------
CODE_STEPS = [2.0 ** -17, 2.0 ** -16, 0.0511, 0.3935, 0.9999, 1.0, 1.023, 3.93, 14.5, 29.0, 31.9,
              100.0, 1022.5]


def _tie(s):
    """a carrier step on a rounding tie of the 2^-53 lattice (the existing generator's ties)"""
    return math.copysign((math.floor(abs(s) / U53) + 0.5) * U53, s)


CARR_STEPS = [0.0, 2.0 ** -60, -2.0 ** -60, 1e-5, -1e-5, 0.45, -0.45, (1.0 - U53) / 2,
              -(1.0 - U53) / 2, _tie(4100.0 / 2.6e6), _tie(-4100.0 / 2.6e6), _tie(33.0 / 2.6e6),
              _tie(-33.0 / 2.6e6), _tie(-0.3)]
assert math.gcd(len(CODE_STEPS), len(CARR_STEPS)) == 1     # cycled together: every pairing occurs
DOPPLER = [1.7e-3, -1.1e-3, 9.3e-6, -2.0e-3, 6.1e-4, -4.0e-5, 0.0]     # mixed signs, cycles/sample
CARR0S = [0.0, 1.0, 1.0 - U53, None, None]                # None: a seeded random phase
CODE0S = [0.0, 1022.9999999, "wrap", None]                # "wrap": wraps on the first add
GAINS = [97, -64, 0, 129, -1, 500, 33, -250, 1]           # |gain| * 250 * 16 = 2e6 << 2^31


def wrap_code0(step, w=0):
    """the code phase whose (w + 1)-th add of `step` is the first to reach 1023"""
    c = 1023.0 - step * (w + 1)
    while oracle.code_brute(c, step, w + 1, 0, 0, 0)[1] == 0:
        c = math.nextafter(c, 1023.0)
    assert 0.0 <= c < 1023.0 and (w == 0 or oracle.code_brute(c, step, w, 0, 0, 0)[1] == 0)
    return c


def rows(nch, code_step, carr_step, gain=GAINS, counters=None, carr0=(None,), code0=(None,),
         tables=None, seed=0, n_nav=8):
    """(blk, nch, nav) for the channel counts `nch`: every family is a sequence cycled over the
    live rows in (block, channel) order, so the rows do not depend on the block length.
    counters: (icode, ibit, iword) triples, None in one for a seeded draw (iword < 40);
    tables: (ca_tbl, nav_tbl) pairs (default seeded); carr0 / code0: None for a seeded draw,
    code0 "wrap" for the phase that wraps on the row's first add."""
    rng = np.random.default_rng(seed)
    nch = np.array(nch, np.int32)
    blk = np.zeros((len(nch), G.MAXCH), G.CHAN_DTYPE)
    nav = rng.integers(0, 1 << 30, size=(n_nav, G.NAV_WORDS), dtype=np.uint32)
    counters = counters or [None]
    i = 0
    for b in range(len(nch)):
        for k in range(nch[b]):
            p = blk[b, k]
            cs = code_step[i % len(code_step)]
            p["code_step"] = cs
            p["carr_step"] = carr_step[i % len(carr_step)]
            x = carr0[i % len(carr0)]
            p["carr0"] = rng.random() if x is None else x
            c = code0[i % len(code0)]
            r = rng.random() * 1023.0
            p["code0"] = r if c is None else wrap_code0(cs) if isinstance(c, str) else c
            cnt = counters[i % len(counters)]
            draw = (rng.integers(0, 20), rng.integers(0, 30), rng.integers(0, 40))
            p["icode"], p["ibit"], p["iword"] = cnt if cnt is not None else draw
            p["gain"] = gain[i % len(gain)]
            t = (rng.integers(0, 32), rng.integers(0, n_nav))
            p["ca_tbl"], p["nav_tbl"] = tables[i % len(tables)] if tables else t
            i += 1
    return blk, nch, nav


def instance_nch(nchp):
    """the instance sweep's channel counts: NCH, a smaller block (an empty one at NCH <= 3), NCH"""
    return [nchp, max(nchp - 3, 0), nchp]


SWEEP_CNT = [None, (19, 29, None), None, None, (19, 29, None)]


def _cnt(rng_seed, cnts):
    """counters with the None iword of a (19, 29, None) entry drawn below 40"""
    r = np.random.default_rng(rng_seed)
    return [c if c is None else (c[0], c[1], int(r.integers(0, 40))) for c in cnts]


def sweep_rows(nchp):
    """instance sweep: code step 0.39, mixed Doppler signs, icode / ibit at 19 / 29 on some rows,
    negative and zero gains"""
    return rows(instance_nch(nchp), [0.3935], DOPPLER, counters=_cnt(nchp, SWEEP_CNT),
                carr0=CARR0S, code0=CODE0S, seed=100 + nchp)


def length_rows(nchp):
    """length sweep: two blocks, the second shorter in channels"""
    return rows([nchp, max(nchp - 2, 1)], [0.3935, 0.0511, 1.023], DOPPLER,
                counters=_cnt(7, SWEEP_CNT), carr0=CARR0S, code0=CODE0S, seed=200 + nchp)


RATE_NCH = [16, 5, 12]


def rate_rows(which):
    """which: an index into CODE_STEPS (that step alone) or "mixed" (every step, across the
    channels and blocks of one call)"""
    cs = CODE_STEPS if which == "mixed" else [CODE_STEPS[which]]
    return rows(RATE_NCH, cs, CARR_STEPS, carr0=CARR0S, code0=CODE0S,
                seed=300 + (99 if which == "mixed" else which))


def many_rows():
    """70 blocks with nch random in 0..16: more than one Stage A wave per channel"""
    r = np.random.default_rng(70)
    nch = r.integers(0, 17, size=70)
    nch[3], nch[68] = 16, 0
    return rows(nch, [0.3935, 1.023], DOPPLER + CARR_STEPS[1:9], counters=_cnt(70, SWEEP_CNT),
                carr0=CARR0S, code0=CODE0S, seed=70)


SUM_CELLS = 8


def sum_rows(one_big):
    """8 channels in one LUT cell per block (equal carr0, a step of 1e-12, one chip stream), the
    cells at j/8 of a cycle, gains +-1000 whose data bits make every product gain * dataBit the
    block's sign: sum |gain| = 8000 is the packed accumulator's limit and both sums sit at their
    extremes, (I, Q) in all four sign pairs over the cells and the two block signs.  one_big: one
    gain of 1001 (sum 8001, the int32 path)."""
    nblk = 2 * SUM_CELLS
    blk, nch, nav = rows([8] * nblk, [0.3935], [1e-12], seed=400, n_nav=2)
    nav[0, :] = 0x3FFFFFFF                      # data bit +1
    nav[1, :] = 0                               # data bit -1
    for b in range(nblk):
        sign = 1 if b < SUM_CELLS else -1
        for k in range(8):
            p = blk[b, k]
            p["carr0"] = (b % SUM_CELLS) / 8.0 + 2.0 ** -11
            p["code0"], p["ca_tbl"] = 511.25, 5
            p["icode"], p["ibit"], p["iword"] = 3, 4, 5
            d = 1 if k % 3 else -1
            p["nav_tbl"] = 0 if d > 0 else 1
            p["gain"] = sign * d * (1001 if one_big and k == 6 else 1000)
    return blk, nch, nav


# ---- the overrun cases: (name, n, wrap sample or None, formats) ---------------------------------
# The row (code0 = 1023 - 0.25 (w + 1), code_step = 0.25, icode 19, ibit 29, iword 59) wraps into
# nav word 60 on the add of sample w (0-based): the oracle returns GSS_E_RANGE when w < n.
OVERRUN_N = 1300
OVERRUN_CASES = [
    ("n2_last", 2, 1, (16, 8)),
    ("n1_never", 1, 1, (16, 8)),
    ("n4_last", 4, 3, (1,)),
    ("n4_never", 4, 4, (1,)),
    ("sample1", OVERRUN_N, 1, (16, 8, 1)),
    ("mid_chunk", OVERRUN_N, 17, (16, 8, 1)),
    ("seg_last_r256", OVERRUN_N, 255, (16, 8, 1)),
    ("seg_first_r256", OVERRUN_N, 256, (16, 8, 1)),
    ("seg_last_r1024", OVERRUN_N, 1023, (16, 8, 1)),
    ("seg_first_r1024", OVERRUN_N, 1024, (16, 8, 1)),
    ("chunk_end_block_last", 1280, 1279, (16, 8)),      # the last chunk of the block is full
    ("chunk_end_block_last_sc01", 1024, 1023, (1,)),    # ... at 512 samples per chunk, R = 1024
    ("block_last", OVERRUN_N, OVERRUN_N - 1, (16, 8, 1)),
    ("never", OVERRUN_N, OVERRUN_N, (16, 8, 1)),
]


def overrun_expect(n, w):
    return E_RANGE if w < n else 0


def overrun_rows(w):
    """three blocks; channel 2 of the middle one is the overrun row wrapping at sample w"""
    blk, nch, nav = rows([5, 4, 6], [0.3935], DOPPLER, counters=[(3, 7, 11)], carr0=CARR0S,
                         seed=500)
    p = blk[1, 2]
    p["code0"], p["code_step"] = 1023.0 - 0.25 * (w + 1), 0.25
    p["icode"], p["ibit"], p["iword"] = 19, 29, 59
    return blk, nch, nav


# every row family the GPU tests use, by name: (blk, nch, nav) and the block lengths it runs at
LENGTHS = [1, 2, 7, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1057, 3073, 16389,
           65537, 262145]
LENGTHS_SC01 = [4, 8, 12, 16, 20, 60, 64, 68, 508, 512, 516, 1020, 1024, 1028, 3076, 16388, 65540,
                262148]
CK_LENGTHS = [1, 7, 8, 9, 257, 1025, 16389]
SEG_R_LENGTHS = [1025, 3073, 16389]
RATE_N = 2100
SWEEP_N = {"device": 1300, "fallback": 600}
MANY_N = 520
SUM_N = 64


def _specs():
    """name -> (maker, its arguments, [block lengths]); builds no rows (and so needs no oracle)"""
    f = {}
    for nchp in range(1, 17):
        f[f"sweep{nchp}"] = (sweep_rows, (nchp,), sorted(set(SWEEP_N.values())))
    for nchp in (3, 13):
        f[f"length{nchp}"] = (length_rows, (nchp,), sorted(set(LENGTHS + LENGTHS_SC01)))
    for i in list(range(len(CODE_STEPS))) + ["mixed"]:
        f[f"rate_{i}"] = (rate_rows, (i,), [RATE_N])
    f["many"] = (many_rows, (), [MANY_N])
    f["sum8000"] = (sum_rows, (False,), [SUM_N])
    f["sum8001"] = (sum_rows, (True,), [SUM_N])
    for name, n, w, _ in OVERRUN_CASES:
        f[f"overrun_{name}"] = (overrun_rows, (w,), [n])
    return f


SPECS = _specs()
FAMILY_NAMES = sorted(SPECS)


@functools.lru_cache(maxsize=None)
def family(name):
    """((blk, nch, nav), [block lengths]) of a named family, built on first use"""
    make, args, lens = SPECS[name]
    return make(*args), lens


def rows_valid(blk, nch, n_ca=32, n_nav=8):
    """gss_synth_host's argument checks (ranges of code0, carr0, steps, counters, table rows)"""
    for b in range(len(nch)):
        if not 0 <= nch[b] <= G.MAXCH:
            return False
        for k in range(nch[b]):
            p = blk[b, k]
            if not (0 <= p["ca_tbl"] < n_ca and 0 <= p["nav_tbl"] < n_nav and
                    0 <= p["ibit"] < 30 and 0 <= p["icode"] < 20 and
                    0 <= p["iword"] < G.NAV_WORDS and 0.0 <= p["code0"] < 1023.0 and
                    0.0 <= p["carr0"] <= 1.0 and 0.0 < p["code_step"] < 1023.0 and
                    -1.0 < p["carr_step"] < 1.0 and p["carr0"] + p["carr_step"] < 2.0):
                return False
    return True


def ck_pos(n):
    return [(j * n) // G.NCK for j in range(G.NCK)]


def checkpoints(blk, nch, n):
    """[nblk, 16, NCK] carrier checkpoints at the samples (j n) // NCK, by brute force
    (oracle.carr_brute_trace), not by the host planner"""
    ck = np.zeros((len(nch), G.MAXCH, G.NCK))
    at = ck_pos(n)
    for b in range(len(nch)):
        for k in range(nch[b]):
            ck[b, k] = oracle.carr_brute_trace(float(blk[b, k]["carr0"]),
                                               float(blk[b, k]["carr_step"]), at)
    return ck


# ---- the device harness -------------------------------------------------------------------------
GUARD_BYTES = 4096


def on_device(dev, blk, nch, ca, nav, n, fmt, ck=None, want_end=False, out_off=0, via="device"):
    """One call of the exact path with everything uploaded by torch.  The output starts out_off
    bytes into a 256-byte aligned buffer and lies, like carr_end, between 0xA5 guard bytes that
    must survive.  via "device": Device.synth_device (no block list, the handle's seg_r);
    "fallback": Device.synth_lin_device with fast all zero, zeroed lin rows and every block in the
    list (R = 256; that entry has no carr_end).  Returns (bytes, carr_end or None, status)."""
    import torch
    dt = torch.device("cuda", 0)
    nblk = len(nch)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)   # noqa: E731
    d_blk = up(np.ascontiguousarray(blk, G.CHAN_DTYPE).view(np.uint8).reshape(-1))
    d_nch = up(np.ascontiguousarray(nch, np.int32))
    d_ca = up(np.ascontiguousarray(ca, np.uint32).view(np.int32))
    d_nav = up(np.ascontiguousarray(nav, np.uint32).view(np.int32))
    d_ck = up(np.ascontiguousarray(ck, np.float64)) if ck is not None else None
    if ck is not None:
        assert ck.shape == (nblk, G.MAXCH, G.NCK)
    nbytes = nblk * G.block_bytes(n, fmt)
    lo = GUARD_BYTES + out_off
    d_out = torch.full((lo + nbytes + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=dt)
    assert d_out.data_ptr() % 256 == 0
    d_st = torch.zeros(1, dtype=torch.int32, device=dt)
    ne = nblk * G.MAXCH
    d_end = torch.full(((ne + 2 * 64) * 8,), GUARD, dtype=torch.uint8, device=dt)
    nch_max = int(np.max(nch))
    ck_ptr = d_ck.data_ptr() if d_ck is not None else 0
    if via == "device":
        end_ptr = d_end.data_ptr() + 64 * 8 if want_end else 0
        dev.synth_device(d_blk.data_ptr(), d_nch.data_ptr(), nch_max, d_ca.data_ptr(), len(ca),
                         d_nav.data_ptr(), len(nav), nblk, n, fmt, d_out.data_ptr() + lo,
                         carr_end_ptr=end_ptr, status_ptr=d_st.data_ptr(), ck_ptr=ck_ptr)
    else:
        assert via == "fallback"
        d_lin = torch.zeros(ne * G.LIN_DTYPE.itemsize, dtype=torch.uint8, device=dt)
        d_fast = torch.zeros(nblk, dtype=torch.int32, device=dt)
        d_fb = up(np.arange(nblk, dtype=np.int32))
        dev.synth_lin_device(d_blk.data_ptr(), d_nch.data_ptr(), nch_max, d_lin.data_ptr(),
                             d_fast.data_ptr(), d_fb.data_ptr(), nblk, d_ca.data_ptr(), len(ca),
                             d_nav.data_ptr(), len(nav), nblk, n, fmt, d_out.data_ptr() + lo,
                             status_ptr=d_st.data_ptr(), ck_ptr=ck_ptr)
    torch.cuda.synchronize(dt)
    o = d_out.cpu().numpy()
    assert np.all(o[:lo] == GUARD), "bytes written before the output"
    assert np.all(o[lo + nbytes:] == GUARD), "bytes written past the output"
    e = d_end.cpu().numpy()
    end = None
    if via == "device" and want_end:
        assert np.all(e[:64 * 8] == GUARD) and np.all(e[(64 + ne) * 8:] == GUARD), \
            "bytes written around carr_end"
        end = e[64 * 8:(64 + ne) * 8].copy().view(np.float64).reshape(nblk, G.MAXCH)
    else:
        assert np.all(e == GUARD)
    return o[lo:lo + nbytes].copy(), end, int(d_st.cpu().numpy()[0])


_want = {}


def want(key, blk, nch, ca, nav, n, fmt):
    """the oracle's (bytes, carr_end, rc), computed once per key and left unchanged"""
    k = (key, n, fmt)
    if k not in _want:
        o, e, rc = oracle.synth(blk, nch, ca, nav, n, fmt, want_carr_end=True)
        o.setflags(write=False)
        e.setflags(write=False)
        _want[k] = (o, e, rc)
    return _want[k]


def check(dev, key, blk, nch, ca, nav, n, fmt, nchp, ck=None, out_off=0, via="device",
          expect_rc=None):
    """One call on the device against oracle.synth(..., want_carr_end=True): the bytes, carr_end
    of the live channels bit for bit (via "device"), status != 0 exactly when the oracle's rc is
    GSS_E_RANGE, Stage B launched once and the fast kernel not at all (via "fallback" launches
    it once over fast == 0, where it renders nothing: the lin rows are zeros), and nch.max() is
    the instance meant.  key names the rows for the oracle cache.  Returns the status."""
    assert int(np.max(nch)) == nchp, "the call selects another kernel instance than meant"
    w_out, w_end, w_rc = want(key, blk, nch, ca, nav, n, fmt)
    assert w_rc in (0, E_RANGE)
    if expect_rc is not None:
        assert w_rc == expect_rc, f"the generator's row is not the case meant (oracle rc {w_rc})"
    dev.timing_reset()
    got, end, status = on_device(dev, blk, nch, ca, nav, n, fmt, ck=ck, want_end=True,
                                 out_off=out_off, via=via)
    tag = f"{key} n={n} fmt={fmt} via={via} off={out_off} ck={ck is not None}"
    assert dev.timing()[0] == 1, f"{tag}: Stage B launches"
    assert dev.timing_lin()[0] == (0 if via == "device" else 1), f"{tag}: fast-kernel launches"
    bad = np.nonzero(got != w_out)[0]
    assert bad.size == 0, f"{tag}: {bad.size} bytes differ, first at {bad[:5]}"
    if end is not None:
        for b in range(len(nch)):
            assert np.array_equal(end[b, :nch[b]].view(np.uint64),
                                  np.asarray(w_end[b, :nch[b]]).view(np.uint64)), \
                f"{tag}: carr_end of block {b}"
    assert (status != 0) == (w_rc == E_RANGE), f"{tag}: status {status}, oracle rc {w_rc}"
    return status
