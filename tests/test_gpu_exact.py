"""The exact render path (gss_anchor_kernel + gss_synth_kernel<NCH, FMT>, csrc/hip/gss_synth.hip)
against the scalar oracle of the reference loop, bit for bit: every kernel instance, the block
lengths around every chunk / segment / workgroup edge, code and carrier steps at the edges of the
chip-window period and of the walks, carrier checkpoints made by brute force, GSS_SEG_R handles,
the packed accumulator's limit and the nav-word overrun status.

Both entries are driven with device pointers (tests/exact_oracle.py): "device" is
gss_synth_device (no block list, the handle's segment length), "fallback" is gss_synth_lin_device
with no certified block (a block list, 256-sample segments).  Every row family used here is
checked on the CPU first (tests/test_exact_inputs.py).
"""
import numpy as np
import pytest

import exact_oracle as X
import gpssim_amd as G

pytestmark = pytest.mark.gpu

VIAS = ["device", "fallback"]
MISALIGNED = {16: 4, 8: 2, 1: 1}          # an output base the header promises nothing about


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ca():
    return G.ca_table()


def fam(name, *_):
    """the family's rows, built once (tests/exact_oracle.py)"""
    return X.family(name)[0]


# ---- all 48 instances ---------------------------------------------------------------------------
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("nchp", range(1, 17))
def test_instance_vs_oracle(dev, ca, nchp, fmt, via):
    """gss_synth_kernel<nchp, fmt>: three blocks with nch = [NCH, max(NCH - 3, 0), NCH] (the
    padding of floors4's operands and of the silent channels), 1300 samples through the plain
    entry and 600 through the fast path's leftover entry"""
    blk, nch, nav = fam(f"sweep{nchp}", X.sweep_rows, nchp)
    X.check(dev, f"sweep{nchp}", blk, nch, ca, nav, X.SWEEP_N[via], fmt, nchp, via=via)


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("nchp", range(1, 17))
def test_instance_with_checkpoints(dev, ca, nchp, via):
    """the SC16 column again with brute-force checkpoints: Stage A's other wave index space"""
    blk, nch, nav = fam(f"sweep{nchp}", X.sweep_rows, nchp)
    n = X.SWEEP_N[via]
    X.check(dev, f"sweep{nchp}", blk, nch, ca, nav, n, 16, nchp, ck=X.checkpoints(blk, nch, n),
            via=via)


# ---- block lengths ------------------------------------------------------------------------------
FMT_LEN = [(f, n) for f in (16, 8) for n in X.LENGTHS] + [(1, n) for n in X.LENGTHS_SC01]


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("nchp", [3, 13])
@pytest.mark.parametrize("fmt,n", FMT_LEN, ids=[f"{f}-{n}" for f, n in FMT_LEN])
def test_lengths_vs_oracle(dev, ca, fmt, n, nchp, via):
    """blocks shorter than GSS_NCK samples, than a staged chunk (32 / 64 / 512 samples), than a
    segment; one sample around each of those edges; a second workgroup (65537 at R = 256, 262145
    at R = 1024); each with an aligned and a misaligned output base"""
    blk, nch, nav = fam(f"length{nchp}", X.length_rows, nchp)
    for off in (0, MISALIGNED[fmt]):
        X.check(dev, f"length{nchp}", blk, nch, ca, nav, n, fmt, nchp, out_off=off, via=via)


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("nchp", [3, 13])
def test_lengths_with_checkpoints(dev, ca, nchp, via):
    """checkpoint positions (j n) // 8 that coincide (n < 8), sit one sample apart, and fall on
    and beside segment starts"""
    blk, nch, nav = fam(f"length{nchp}", X.length_rows, nchp)
    for n in X.CK_LENGTHS:
        X.check(dev, f"length{nchp}", blk, nch, ca, nav, n, 16, nchp,
                ck=X.checkpoints(blk, nch, n), via=via)


# ---- rates --------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("fmt", [16, 1])
@pytest.mark.parametrize("which", list(range(len(X.CODE_STEPS))) + ["mixed"])
def test_rates_vs_oracle(dev, ca, which, fmt, via):
    """every code step alone (ks_max, and so the chip-window period, from that step: 65536 below
    29 / 65536, floor(29 / ks) down to 1, 1 above 29; the general code walk below 2^-16) and all
    of them mixed over the channels and blocks of one call (ks_max and the anchor wave's choice of
    walk come from one row), with the carrier steps 0, +-2^-60 ... +-(1 - 2^-53) / 2 and rounding
    ties, carr0 in {0, 1, 1 - 2^-53}, code0 in {0, 1022.9999999, wraps on the first add}"""
    blk, nch, nav = fam(f"rate_{which}", X.rate_rows, which)
    X.check(dev, f"rate_{which}", blk, nch, ca, nav, X.RATE_N, fmt, max(X.RATE_NCH), via=via)


# ---- many blocks: more than one Stage A wave per channel -----------------------------------------
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("with_ck", [False, True])
def test_seventy_blocks(dev, ca, with_ck, via):
    blk, nch, nav = fam("many", X.many_rows)
    ck = X.checkpoints(blk, nch, X.MANY_N) if with_ck else None
    X.check(dev, "many", blk, nch, ca, nav, X.MANY_N, 16, 16, ck=ck, via=via)


# ---- GSS_SEG_R ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_r", [256, 512, 2048])
def test_seg_r_handles(ca, monkeypatch, seg_r):
    """a fresh handle under GSS_SEG_R: lengths with a ragged last segment at every R.  That the
    handle took the value shows in its anchor sets: reserved for one block of 31 R samples they
    hold 32 slots per channel, so a render call of 31 R samples passes the size check (and stops
    at the nch_max given as 17, before any launch) and one of 31 R + 1 samples does not."""
    import torch
    monkeypatch.setenv("GSS_SEG_R", str(seg_r))
    d = G.Device(0)
    try:
        d.reserve(1, 31 * seg_r)
        t = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        for n, code in ((31 * seg_r, -1), (31 * seg_r + 1, -6)):      # GSS_E_ARG, GSS_E_STATE
            with pytest.raises(G.GssError) as e:
                d.render_device(0, t.data_ptr(), t.data_ptr(), 17, t.data_ptr(), 32, t.data_ptr(),
                                8, 1, n, 16, t.data_ptr())
            assert e.value.code == code, (n, str(e.value))
        blk, nch, nav = fam("length13")
        for n in X.SEG_R_LENGTHS:
            for fmt in (16, 8):
                X.check(d, "length13", blk, nch, ca, nav, n, fmt, 13, via="device")
    finally:
        d.close()


def test_unsupported_carrier_row_is_refused(dev, ca):
    """carr0 == 1.0 with carr_step == 1 - 2^-53: the first sum rounds to 2.0, outside what the
    kernels' r - floor(r) covers; gss_synth_host refuses the row (include/gpssim_amd.h)"""
    blk, nch, nav = X.rows([1], [0.3935], [1.0 - X.U53], carr0=[1.0])
    assert not X.rows_valid(blk, nch)
    with pytest.raises(G.GssError) as e:
        dev.synth_host(blk, nch, ca, nav, 64, 16)
    assert e.value.code == -1
    blk[0, 0]["carr0"] = 1.0 - X.U53                   # the largest sum that is supported
    assert X.rows_valid(blk, nch)
    X.check(dev, "carr_sum_max", blk, nch, ca, nav, 600, 16, 1)


# ---- sums ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("one_big", [False, True], ids=["sum8000", "sum8001"])
def test_sum_extremes_vs_oracle(dev, ca, one_big, fmt, via):
    """sum |gain| = 8000 (the packed int64 accumulator at its limit, with the borrow between its
    I and Q halves) and 8001 (the int32 path), both sums at their extremes in all four sign pairs"""
    name = "sum8001" if one_big else "sum8000"
    blk, nch, nav = fam(name, X.sum_rows, one_big)
    X.check(dev, name, blk, nch, ca, nav, X.SUM_N, fmt, 8, via=via)


# ---- the overrun status -------------------------------------------------------------------------
OVERRUN = [(c, f) for c in X.OVERRUN_CASES for f in c[3]]


@pytest.mark.parametrize("via", VIAS + ["host"])
@pytest.mark.parametrize("case,fmt", OVERRUN, ids=[f"{c[0]}-{f}" for c, f in OVERRUN])
def test_overrun_status(dev, ca, case, fmt, via):
    """GSS_E_RANGE exactly when the oracle reports it: the wrap into nav word 60 made by the add
    of sample 1, mid-chunk, of a segment's last and the next one's first sample (both segment
    lengths), of the block's last sample (in a ragged and in a full last chunk), and one sample
    past the block (never); the bytes are the oracle's in every case"""
    name, n, w, _ = case
    blk, nch, nav = fam(f"overrun_{name}", X.overrun_rows, w)
    rc = X.overrun_expect(n, w)
    if via != "host":
        status = X.check(dev, f"overrun_{name}", blk, nch, ca, nav, n, fmt, 6, via=via,
                         expect_rc=rc)
        assert (status != 0) == (rc == X.E_RANGE)
        return
    want, _, w_rc = X.want(f"overrun_{name}", blk, nch, ca, nav, n, fmt)
    assert w_rc == rc
    if rc:
        with pytest.raises(G.GssError) as e:
            dev.synth_host(blk, nch, ca, nav, n, fmt)
        assert e.value.code == X.E_RANGE
    else:
        assert np.array_equal(dev.synth_host(blk, nch, ca, nav, n, fmt), want)
