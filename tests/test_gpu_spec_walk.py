"""The run-ahead carrier walks on the GPU (csrc/hip/gss_producers.hip: gss_spec_kernel, the
row-shared cycle cache of sc_seg_walk, gss_spec_rec_kernel) on the synthetic rows of
tests/spec_oracle.py: against the host's walks (gss_spec_host, itself checked on the same rows by
tests/test_spec_walk.py) bit for bit, and on their own against brute force (check_walks: every
segment's interval of exact start translations at both of its ends).  Row counts that leave a
workgroup half or wholly idle, rows that arrive with wrong guesses, the records' 8-byte tail and
links across the 64-row workgroups, and the nav rows in uneven pieces.  Every device buffer sits
between 0xA5 guard bytes, which must survive."""
import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import spec_oracle as O
from spec_oracle import _spec_walks_agree, check_walks

pytestmark = pytest.mark.gpu

GUARD = 256                                   # keeps the payload's 16-byte alignment
IN, SP, REC = G.SPEC_IN_DTYPE, G.SPEC_DTYPE, G.SPEC_REC_DTYPE


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def guarded(nbytes, data=None):
    """a device buffer of nbytes between guards, all 0xA5 or holding data: (tensor, pointer)"""
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if data is not None:
        b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert b.size == nbytes
        t[GUARD:GUARD + nbytes] = torch.from_numpy(b.copy()).cuda()
    assert (t.data_ptr() + GUARD) % 16 == 0
    return t, t.data_ptr() + GUARD


def payload(t, dtype):
    h = t.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[-GUARD:] == 0xA5).all(), "wrote outside"
    return h[GUARD:-GUARD].copy().view(dtype)


def device_walks(dev, gi, nrow, n):
    """Device.spec_device over the first nrow of the rows gi: (all rows as they come back, all
    walks: 0xA5 bytes where nothing was written)"""
    import torch
    gi = np.ascontiguousarray(gi, IN).reshape(-1)
    t_in, p_in = guarded(gi.nbytes, gi)
    t_sp, p_sp = guarded(len(gi) * SP.itemsize)
    dev.spec_device(p_in, nrow, n, p_sp)
    torch.cuda.synchronize()
    return payload(t_in, IN), payload(t_sp, SP)


def device_records(dev, gi, nrow, n):
    """Device.spec_records_device over the first nrow rows: (rows in, unchanged; the device's
    rows with its guesses; its walks; the records), each of len(gi) rows"""
    import torch
    gi = np.ascontiguousarray(gi, IN).reshape(-1)
    t_in, p_in = guarded(gi.nbytes, gi)
    t_din, p_din = guarded(gi.nbytes)
    t_sp, p_sp = guarded(len(gi) * SP.itemsize)
    t_rec, p_rec = guarded(len(gi) * REC.itemsize)
    dev.spec_records_device(p_in, nrow, n, p_din, p_sp, p_rec)
    torch.cuda.synchronize()
    return payload(t_in, IN), payload(t_din, IN), payload(t_sp, SP), payload(t_rec, REC)


def untouched(a, nrow):
    return bool((a[nrow:].view(np.uint8) == 0xA5).all())


_host = {}


def host(key, gi, n):
    """the host's guesses and walks of the rows gi, computed once per key and left unchanged:
    (rows with the guesses, walks)"""
    if key not in _host:
        g = np.ascontiguousarray(gi, IN).reshape(-1).copy()
        _host[key] = (g, G.spec_host(g, n, threads=8))
    return _host[key]


def agree_and_sound(got_in, got, want_in, want, nrow, n, kw, may_void=None):
    """the assertions every walk test makes over rows [0, nrow); returns the translation checks"""
    assert got_in[:nrow].tobytes() == want_in[:nrow].tobytes(), kw
    checks = check_walks(want_in[:nrow], got[:nrow], n, may_void)      # on their own, first
    print(f"{kw}: {checks} translation checks")
    _spec_walks_agree(got[:nrow], want[:nrow], want_in[:nrow], kw)
    idle = want_in[:nrow]["s"] == 0                    # padding rows: no walk, the same bytes
    assert got[:nrow][idle].tobytes() == want[:nrow][idle].tobytes(), kw
    return checks


@pytest.mark.parametrize("n,seed,count", [(33, 1, 160), (33, 2, 160), (4100, 1, 160),
                                          (4100, 2, 160), (260000, 1, 160), (260000, 2, 160),
                                          (2000000, 1, 32)])
def test_device_walks_synthetic(dev, n, seed, count):
    """rows with k = 0: the lanes guess the segment starts (written back equal to the host's) and
    walk them; 160 and 32 rows are taken channel-major (spec_row_of)"""
    gi = O.spec_in(O.rows(seed, count))
    want_in, want = host(("syn", n, seed, count), gi, n)
    got_in, got = device_walks(dev, gi, count, n)
    assert agree_and_sound(got_in, got, want_in, want, count, n, (n, seed)) > 0
    if n >= 4100:
        assert np.any(want_in["k"] == 1) and np.any(want_in["k"] == G.SPEC_K)


def test_device_walks_power_of_two_lattice(dev):
    """LATTICE_ROWS (spec_oracle): the segments whose margins leave their own start out report no
    interval on the device as on the host, with the exact end"""
    n = 4100
    gi = O.spec_in(O.LATTICE_ROWS)
    want_in, want = host(("lattice",), gi, n)
    got_in, got = device_walks(dev, gi, len(gi), n)
    agree_and_sound(got_in, got, want_in, want, len(gi), n, "lattice")
    seg = got["seg"]
    kept = seg["dlo"] <= seg["dhi"]
    assert np.all((seg["dlo"][kept] <= 0) & (seg["dhi"][kept] >= 0))


def counted_rows():
    """104 rows at n = 4,100, some of them padding (s = 0): row 4 of every five beside a live row
    of its workgroup, rows 6 and 7 a whole workgroup where rows are taken in order, rows 32 and 48
    one where 80 rows are taken channel-major"""
    gi = O.spec_in(O.rows(3, 104))
    i = np.arange(len(gi))
    idle = (i % 5 == 4) | np.isin(i, (6, 7, 32, 48))
    gi["s"][idle] = 0.0
    gi["g"][idle] = 0.0
    fast = int(np.flatnonzero(np.abs(gi["s"]) > 0.01)[0])      # row 0: one with many wraps
    gi[[0, fast]] = gi[[fast, 0]]
    return gi


@pytest.mark.parametrize("nrow", [1, 2, 3, 15, 17, 31, 80, 100])
def test_device_walks_row_counts(dev, nrow):
    """both branches of spec_row_of (80 rows: channel-major; the others in order), a last
    workgroup with one live row (odd counts), workgroups of padding rows only and of one padding
    and one live row; the rows and walks past nrow stay as they were"""
    n = 4100
    gi = counted_rows()
    want_in, want = host(("cnt",), gi, n)
    got_in, got = device_walks(dev, gi, nrow, n)
    assert got_in[nrow:].tobytes() == gi[nrow:].tobytes()
    assert untouched(got, nrow)
    checks = agree_and_sound(got_in, got, want_in, want, nrow, n, nrow)
    assert checks > 0
    if nrow >= 8:
        assert np.any(want_in[:nrow]["s"] == 0)


@pytest.mark.parametrize("n", [4100, 260000])
@pytest.mark.parametrize("mode", ["start", "segments", "counts"])
def test_device_walks_given_guesses(dev, n, mode):
    """Rows that arrive with guesses (k >= 1), wrong as in
    test_host_plane.py::test_speculative_chain_exact_with_wrong_guesses: the start 1e-4 cycle off,
    the segment starts one sample late from values 3e-7 off, or the segments cut to 1..3.  The
    device leaves such rows as they are and walks the segments as given, like the host; a
    segment's claim is about the segment as given, so it holds from values off the post-wrap
    lattice too (on the host: checked with these rows while this test was written)."""
    base_in, _ = host(("syn", n, 4, 160), O.spec_in(O.rows(4, 160)), n)
    g = base_in.copy()
    rng = np.random.default_rng(7)
    if mode == "start":
        g["g"] = np.mod(g["g"] + 1e-4, 1.0)
    elif mode == "segments":
        moved = g["P"][:, 1:] > 0
        g["P"][:, 1:] += moved
        g["W"][:, 1:] = np.where(moved, np.mod(g["W"][:, 1:] + 3e-7, 1.0), 0.0)
    else:
        g["k"] = np.minimum(g["k"], rng.integers(1, 4, size=len(g)))
    assert np.all(g["k"] >= 1)
    want_in, want = host(("given", n, mode), g, n)
    assert want_in.tobytes() == g.tobytes()              # the host guesses nothing either
    got_in, got = device_walks(dev, g, len(g), n)
    assert agree_and_sound(got_in, got, want_in, want, len(g), n, (n, mode),
                           O.on_lattice(base_in)) > 0


def linked_rows(n):
    """200 generator rows as blocks of 16 slots: row i follows row i - 16 (pad), its start the
    line's prediction from that row's, so that links can hold; a few rows without a previous row
    (pad -1), a few with pad = i and i + 1 (invalid: no link), a few padding rows"""
    rows = O.rows(5, 200)
    gi = O.spec_in(rows)
    i = np.arange(len(gi))
    idle = i % 17 == 11
    gi["s"][idle] = 0.0
    gi["g"][idle] = 0.0
    for r in range(16, len(gi)):
        p = r - 16
        gi["pad"][r] = p
        if gi["s"][p] != 0 and gi["s"][r] != 0 and r % 13 != 12 and r % 11 != 10:
            v = gi["g"][p] + n * gi["s"][p]
            v -= np.floor(v)
            gi["g"][r] = v if 0.0 <= v < 1.0 else 0.0
    gi["pad"][i % 9 == 3] = -1
    own = i % 10 == 7
    gi["pad"][own] = i[own]
    nxt = i % 14 == 5
    gi["pad"][nxt] = i[nxt] + 1
    return gi


@pytest.mark.parametrize("n", [4100, 260000])
@pytest.mark.parametrize("nrow", [1, 63, 64, 65, 100, 200])
def test_device_records_tail_and_links(dev, n, nrow):
    """gss_spec_records_device: the records' 16-byte stores (whole workgroups of 64 rows) and
    8-byte tail, links to a row of the workgroup before, and pads that give no link; the records
    equal the host's over the device's own walks byte for byte, the device's rows the host's
    guesses, and nothing past nrow is written"""
    gi = linked_rows(n)
    want_in, want = host(("rec", n), gi, n)
    got_in, d_in, walks, rec = device_records(dev, gi, nrow, n)
    assert got_in.tobytes() == gi.tobytes()
    assert d_in[:nrow].tobytes() == want_in[:nrow].tobytes()
    assert untouched(d_in, nrow) and untouched(walks, nrow) and untouched(rec, nrow)
    _spec_walks_agree(walks[:nrow], want[:nrow], want_in[:nrow], (n, nrow))
    want_rec = G.spec_records(d_in[:nrow], walks[:nrow], n)
    live = gi[:nrow]["s"] != 0
    assert rec[:nrow][live].tobytes() == want_rec[live].tobytes()
    assert rec[:nrow].tobytes() == want_rec.tobytes()
    i = np.arange(nrow)
    pad = gi[:nrow]["pad"]
    linked = (rec[:nrow]["ok"] & 2) != 0
    assert not np.any(linked & ((pad < 0) | (pad >= i)))
    assert np.all((rec[:nrow]["ok"] >> 2)[linked] == (i - pad)[linked])
    if nrow >= 100:                                      # links across the 64-row boundary
        assert np.any(linked[64:80]), rec[64:80]["ok"]


def test_nav_rows_in_uneven_pieces(dev):
    """gss_nav_rows_device in three launches cut off the 64-row workgroups (after row 1 and 65
    rows before the end) and one of no rows: the host plane's table word for word"""
    import torch
    s = G.Scenario(NAV, llh=LOC, duration=300.0)
    s.all_blocks(batch=500, threads=4)
    src, want = s.nav_sources(), s.nav_table()
    s.close()
    assert len(src) == len(want) > 66
    t_src, p_src = guarded(src.nbytes, src)
    t_rows, p_rows = guarded(want.nbytes)
    cuts = [0, 1, len(src) - 65, len(src)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        dev.nav_rows_device(p_src + a * G.NAV_SRC_DTYPE.itemsize, a, b - a, p_rows)
        dev.nav_rows_device(p_src + b * G.NAV_SRC_DTYPE.itemsize, b, 0, p_rows)
    torch.cuda.synchronize()
    assert payload(t_src, np.uint8).tobytes() == src.tobytes()
    got = payload(t_rows, np.uint32).reshape(want.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
