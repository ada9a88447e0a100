"""GPU parity of the fast path where a wave makes the records of its four chunks in one pass
(gss_lin_kernel: lane 16 c + k makes chunk c of channel k, the render loop takes the rows to load
ahead from those lanes): the shapes at which the chunk indexing of a wave can go wrong, against
the scalar oracle, byte for byte, at all three formats.

Block lengths.  A wave renders 4 chunks of 1,024 samples and a workgroup 4 waves, so what matters
is how the block ends inside its last workgroup and last wave.  The proof certifies a channel only
from about 230,200 samples per block on (63 zs + 3 <= 31 chips at the block length's chip advance;
a synthetic block of 229,000 samples is never certified), so the shapes sit on the first
workgroup boundaries above that, 14 and 15 workgroups of 16,384:

    n         last workgroup             last wave
    230,400   1 wave                     exactly 1 chunk
    231,425   1 wave                     2 chunks + 1 sample
    233,472   1 wave, full               -
    233,473   2 waves                    1 sample
    245,760   full (the block ends on a workgroup boundary)
    245,761   1 wave                     1 sample
    250,000   2 waves                    ragged

Every block of every case is certified (asserted: no block may fall back to the exact path), with
1, 2, 3, 11, 12 and 16 channels, so that a chunk ends with a pair, with a lone last channel after
pairs and with a lone channel alone.  The gain changes of these inputs (data-bit edges, about a
hundred per case) fall in all four chunk positions of a wave, which is asserted from the lines so
that the coverage cannot get lost silently; boundary_params adds patched samples in all four
chunk positions, and one case has blocks of 0 and 1 channels alone, where the rows to load ahead
have no neighbour.
-b 1 packs 8 I/Q bits per byte and takes only block lengths that are multiples of 4
(gss_block_bytes), so at -b 1 each length is rounded up to the next one (_len: a 1-sample tail
becomes a 4-sample one); the parameters keep the seed of the table's length.
"""
import numpy as np
import pytest

from test_linearize import boundary_params, synth_params

import gpssim_amd as G
import oracle

pytestmark = pytest.mark.gpu

SEG, CHUNK = 4096, 1024
LENGTHS = [230400, 231425, 233472, 233473, 245760, 245761, 250000]
NCH = [1, 2, 3, 11, 12, 16]
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


def chunk_positions(pos, n):
    """the chunk of its wave segment (0..3) each listed sample falls in; unused entries, entries
    past the block and (for gain schedules) the entry at sample 0 left out"""
    p = np.asarray(pos).reshape(-1)
    p = p[(p > 0) & (p < n)]
    return (p % SEG) // CHUNK


def lengths_case(n, fmt, nchv=NCH):
    """the inputs of one length: certified throughout, gain changes in every chunk position"""
    m = _len(n, fmt)
    rng = np.random.default_rng(n)
    blk, nch, nav = synth_params(rng, len(nchv), nchv, m)
    lin, fast = G.linearize(blk, nch, nav, m)
    return m, blk, nch, nav, lin, fast


def _run(dev, blk, nch, nav, n, fmt):
    ca = G.ca_table()
    want, rc = oracle.synth(blk, nch, ca, nav, n, fmt)
    assert rc == 0
    dev.timing_reset()
    got = dev.synth_host(blk, nch, ca, nav, n, fmt)
    assert dev.timing_lin()[0] == 1                    # the fast kernel ran
    _same(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("n", LENGTHS)
def test_chunks_last_wave_shapes(dev, fmt, n):
    m, blk, nch, nav, lin, fast = lengths_case(n, fmt)
    assert fast.all(), fast
    used = [lin["gpos"][b, :nch[b]] for b in range(len(nch))]
    where = np.concatenate([chunk_positions(g, m) for g in used])
    assert set(where.tolist()) == {0, 1, 2, 3}, np.bincount(where, minlength=4)
    _run(dev, blk, nch, nav, m, fmt)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_chunks_patches_in_every_chunk_position(dev, fmt):
    """boundary_params at its defaults: code wraps that start data bits and samples on LUT cell
    boundaries, 19 of 36 blocks patched, the patches in all four chunk positions"""
    blk, nch, nav, n = boundary_params()
    lin, fast = G.linearize(blk, nch, nav, n)
    assert fast.sum() == 36 and len(fast) == 36, fast
    ppos = lin["ppos"][:, 0]
    assert int((ppos != I32MAX).any(axis=1).sum()) == 19
    assert set(chunk_positions(ppos, n).tolist()) == {0, 1, 2, 3}
    _run(dev, blk, nch, nav, n, fmt)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_chunks_lone_and_empty_blocks(dev, fmt):
    """blocks of 0 and 1 channels alone: a lone channel's rows to load ahead are its own of the
    next chunk, an empty block loads none"""
    m, blk, nch, nav, lin, fast = lengths_case(LENGTHS[0], fmt, [0, 1, 1, 0, 1, 0])
    assert fast.all(), fast
    _run(dev, blk, nch, nav, m, fmt)
