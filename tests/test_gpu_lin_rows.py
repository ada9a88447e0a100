"""GPU parity of the fast path where the segment rows are built inside gss_lin_kernel: the shapes at
which the row indexing of a workgroup (4 wave segments x up to 16 channels, one row per lane of
its first wave) can go wrong, against the scalar oracle, byte for byte, at all three formats.

Block lengths.  A workgroup renders 4 segments of 4,096 samples, so what matters is what is left
for the last workgroup of a block: 4,100 samples (its waves 2 and 3 past the end), exactly 16,384
(a full workgroup), 16,390 (one more workgroup with a single 6-sample segment), 20,483 (ragged,
odd).  The proof cannot certify a channel at those lengths themselves: the chunk window table
takes the chip advance per sample from the block length (gss_lin_wstep16: 102,300 / n_per_blk
chips per sample, the reference's 10 blocks per second) and a step's 64 lanes must fit a 32-chip
window (GSS_LIN_WIN_OK: 63 zs + 3 <= 31 chips), which needs n_per_blk >= about
230,200 (102,300 / (28 / 63) = 230,175 at zero Doppler; 14 x 16,384 + 6 is not certified).  So
* the lengths themselves run with every channel block on the exact path and the empty block
  (nch = 0) on the fast kernel (TAILS_SHORT: fast == [0, 0, 0, 1], asserted), and
* the same tails after 14 or 15 full workgroups (TAILS: 14 x 16,384 + 4,100 = 233,476,
  15 x 16,384 = 245,760, 245,766, 14 x 16,384 + 4,099 = 233,475; the smallest such lengths above
  the bound) run certified, every block on the fast kernel.
-b 1 packs 8 I/Q bits per byte and takes only block lengths that are multiples of 4
(gss_block_bytes), so at -b 1 each length is rounded up to the next one (_len: the 6-sample
segment becomes an 8-sample one, 20,483 becomes 20,484).
"""
import numpy as np
import pytest

from test_linearize import boundary_params, synth_params

import gpssim_amd as G
import oracle

pytestmark = pytest.mark.gpu

WG = 4 * 4096
TAILS_SHORT = [4100, 16384, 16390, 20483]
TAILS = [14 * WG + 4100, 15 * WG, 15 * WG + 6, 14 * WG + 4099]
NCH = [1, 12, 16, 0]
I32MAX = np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def _len(n, fmt):
    return (n + 3) & ~3 if fmt == 1 else n


def _same(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:5]}"


@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("n", TAILS)
def test_rows_last_workgroup_shapes(dev, fmt, n):
    n = _len(n, fmt)
    rng = np.random.default_rng(n)
    blk, nch, nav = synth_params(rng, len(NCH), NCH, n)
    ca = G.ca_table()
    _, fast = G.linearize(blk, nch, nav, n)
    assert fast.sum() == len(NCH), fast
    want, rc = oracle.synth(blk, nch, ca, nav, n, fmt)
    assert rc == 0
    dev.timing_reset()
    got = dev.synth_host(blk, nch, ca, nav, n, fmt)
    assert dev.timing_lin()[0] == 1                    # the fast kernel ran
    _same(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("n", TAILS_SHORT)
def test_rows_short_blocks(dev, fmt, n):
    """the lengths themselves: no channel can be certified there (module docstring), the empty
    block takes the fast kernel (one or two workgroups, waves past the end, no rows)"""
    n = _len(n, fmt)
    rng = np.random.default_rng(n)
    blk, nch, nav = synth_params(rng, len(NCH), NCH, n, fs=2.6e6)
    ca = G.ca_table()
    _, fast = G.linearize(blk, nch, nav, n)
    assert list(fast) == [0, 0, 0, 1]
    want, rc = oracle.synth(blk, nch, ca, nav, n, fmt)
    assert rc == 0
    dev.timing_reset()
    got = dev.synth_host(blk, nch, ca, nav, n, fmt)
    assert dev.timing_lin()[0] == 1
    _same(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_rows_mixed_batch(dev, fmt):
    """a rejected block (a code step too large for the chip window) between certified ones: its
    workgroups return before the set-up, the exact path renders it in the same call"""
    n = _len(TAILS[2], fmt)
    rng = np.random.default_rng(16390)
    blk, nch, nav = synth_params(rng, 4, [12, 16, 1, 16], n)
    blk[1, 3]["code_step"] = 0.9
    ca = G.ca_table()
    _, fast = G.linearize(blk, nch, nav, n)
    assert list(fast) == [1, 0, 1, 1]
    want, _ = oracle.synth(blk, nch, ca, nav, n, fmt)
    dev.timing_reset()
    got = dev.synth_host(blk, nch, ca, nav, n, fmt)
    assert dev.timing_lin()[0] == 1
    _same(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_rows_patches_and_gain_changes(dev, fmt):
    """boundary_params: code wraps that start data bits (gain changes inside segments) and
    patched samples, at a length whose last workgroup holds one 6-sample segment"""
    n = _len(TAILS[2], fmt)
    blk, nch, nav, _ = boundary_params(nb=14, n=n, fs=10.0 * n)
    keep = blk["code0"][:, 0] >= 0.0                    # (its wrap can lie past this rate's reach)
    blk, nch = blk[keep], nch[keep]
    lin, fast = G.linearize(blk, nch, nav, n)
    ok = fast.astype(bool)
    assert fast.sum() >= 10 and fast.sum() >= len(fast) - 1, fast
    assert (lin["ppos"][ok] != I32MAX).any()
    assert (lin["gpos"][ok][:, 0, 1] != I32MAX).any()
    ca = G.ca_table()
    want, _ = oracle.synth(blk, nch, ca, nav, n, fmt)
    dev.timing_reset()
    got = dev.synth_host(blk, nch, ca, nav, n, fmt)
    assert dev.timing_lin()[0] == 1
    _same(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_rows_inputs_rewritten_in_place(dev, fmt):
    """two gss_synth_lin_device calls on the same device buffers, the rows (blk, nch, lin, fast,
    the exact path's list) overwritten in place with another scenario's between them: nothing
    derived from the first call's inputs may survive into the second"""
    import torch
    dev_t = torch.device("cuda", 0)
    n = TAILS[0]
    ca = G.ca_table()
    sets = []
    for seed, nchv, reject in [(1, [1, 12, 16, 0], None), (2, [16, 3, 12, 7], 2)]:
        rng = np.random.default_rng(seed)
        blk, nch, nav = synth_params(rng, 4, nchv, n)
        if reject is not None:
            blk[reject, 1]["code_step"] = 0.9
        lin, fast = G.linearize(blk, nch, nav, n)
        assert fast.sum() == 4 - (reject is not None), fast
        fb = np.nonzero(fast == 0)[0].astype(np.int32)
        want, _ = oracle.synth(blk, nch, ca, nav, n, fmt)
        sets.append((blk, nch, nav, lin, fast, fb, want))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev_t)   # noqa: E731
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)  # noqa: E731
    blk, nch, nav, lin, fast, fb, _ = sets[0]
    d_blk, d_nch, d_nav = t(raw(blk)), t(nch), t(nav.view(np.int32))
    d_lin, d_fast, d_fb = t(raw(lin)), t(fast), t(np.zeros(4, np.int32))
    d_ca = t(ca.view(np.int32))
    out = torch.empty(4 * G.block_bytes(n, fmt), dtype=torch.uint8, device=dev_t)
    stream = torch.cuda.current_stream(dev_t).cuda_stream
    ptrs = [x.data_ptr() for x in (d_blk, d_nch, d_nav, d_lin, d_fast, d_fb)]
    for i, (blk, nch, nav, lin, fast, fb, want) in enumerate(sets):
        if i:
            d_blk.copy_(t(raw(blk)))
            d_nch.copy_(t(nch))
            d_nav.copy_(t(nav.view(np.int32)))
            d_lin.copy_(t(raw(lin)))
            d_fast.copy_(t(fast))
            d_fb[:len(fb)].copy_(t(fb))
            out.zero_()
        assert ptrs == [x.data_ptr() for x in (d_blk, d_nch, d_nav, d_lin, d_fast, d_fb)]
        dev.synth_lin_device(d_blk.data_ptr(), d_nch.data_ptr(), int(nch.max()),
                             d_lin.data_ptr(), d_fast.data_ptr(), d_fb.data_ptr(), len(fb),
                             d_ca.data_ptr(), len(ca), d_nav.data_ptr(), len(nav), len(nch), n,
                             fmt, out.data_ptr(), stream=stream)
        torch.cuda.synchronize(dev_t)
        _same(out.cpu().numpy(), want)
