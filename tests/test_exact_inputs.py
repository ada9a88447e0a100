"""CPU checks of every row family tests/test_gpu_exact.py gives the exact render path, before any
of them goes near a GPU (tests/exact_oracle.py builds them).

Stage A runs common/gss_phase.h on the device; its host build (tests/helpers/walk_check.c) must
end on these rows and equal brute force at every segment start, for both segment lengths the
product uses (256: the fast path's leftovers, 1024: the plain entry) and for the GSS_SEG_R values
the GPU file opens handles with.  A walk that does not end shows here, not on a shared machine.
"""
import numpy as np
import pytest

import exact_oracle as X
import gpssim_amd as G
import oracle
from conftest import walk_lib

FAM = X.FAMILY_NAMES            # rows are built inside the tests: collection needs no oracle
SEG_RS = (256, 512, 1024, 2048)


def _uniq(blk, nch, fields):
    seen = {}
    for b in range(len(nch)):
        for k in range(nch[b]):
            seen.setdefault(tuple(blk[b, k][f].item() for f in fields), (b, k))
    return list(seen)


def _code_trace(c0, cs, cnt, n, step):
    """brute-force code state at every multiple of `step` below n"""
    out = []
    c, (a, b, d) = c0, cnt
    for j in range((n + step - 1) // step):
        if j:
            c, a, b, d = oracle.code_brute(c, cs, step, a, b, d)
        out.append((c, a | (b << 8) | (d << 16)))
    return out


@pytest.mark.parametrize("name", FAM)
def test_rows_pass_the_argument_checks(name):
    (blk, nch, nav), lens = X.family(name)
    assert X.rows_valid(blk, nch, n_nav=len(nav))
    assert all(n >= 1 for n in lens)
    gmax = int(np.abs(blk["gain"]).max())
    assert gmax * 250 * 16 < 2 ** 28              # the oracle's int sums stay far from overflow


@pytest.mark.parametrize("name", FAM)
def test_host_carrier_walks_equal_brute_force(name):
    """gss_seg_states as Stage A's carrier waves call it -- whole block, and the GSS_NCK
    sub-chains from brute-force checkpoints -- at every segment start and at the block end"""
    W = walk_lib()
    (blk, nch, _), lens = X.family(name)
    for x0, s in _uniq(blk, nch, ("carr0", "carr_step")):
        for n in lens:
            pos = X.ck_pos(n) + [n]
            ck = oracle.carr_brute_trace(x0, s, pos[:-1])
            end_w = oracle.carr_brute(x0, s, n)
            for R in SEG_RS if n > 256 else (256, 1024):
                nseg = (n + R - 1) // R
                at = np.arange(nseg, dtype=np.int64) * R
                want = oracle.carr_brute_trace(x0, s, at)
                ox = np.full(nseg + 1, np.nan)
                end = W.wc_seg_states(x0, s, 0, 0, 0, n, R, nseg, 1, ox.ctypes.data, None)
                assert np.array_equal(ox[:nseg].view(np.uint64), want.view(np.uint64)), \
                    (x0, s, n, R)
                assert end == end_w, (x0, s, n, R)
                ox2 = np.full(nseg + 1, np.nan)
                for j in range(G.NCK):
                    e2 = W.wc_seg_states(ck[j], s, 0, 0, pos[j], pos[j + 1], R, nseg,
                                         int(j == G.NCK - 1), ox2.ctypes.data, None)
                assert np.array_equal(ox2[:nseg].view(np.uint64), want.view(np.uint64)), \
                    (x0, s, n, R, "ck")
                assert e2 == end_w, (x0, s, n, R, "ck")


@pytest.mark.parametrize("name", FAM)
def test_host_code_walks_equal_brute_force(name):
    """the code chain with its counters at every segment start: the general walk (a wave with any
    step below 2^-16 takes it for all its lanes) and the branch-free form for steps >= 2^-16"""
    W = walk_lib()
    (blk, nch, _), lens = X.family(name)
    for c0, cs, a, b, d in _uniq(blk, nch, ("code0", "code_step", "icode", "ibit", "iword")):
        cnt0 = a | (b << 8) | (d << 16)
        for n in lens:
            tr = _code_trace(c0, cs, (a, b, d), n, 256)
            for R in SEG_RS if n > 256 else (256, 1024):
                nseg = (n + R - 1) // R
                want = tr[::R // 256]
                assert len(want) == nseg
                wx = np.array([t[0] for t in want])
                wc = np.array([t[1] for t in want], np.uint32)
                ox = np.full(nseg + 1, np.nan)
                oc = np.zeros(nseg + 1, np.uint32)
                W.wc_seg_states(c0, cs, 1, cnt0, 0, n, R, nseg, 0, ox.ctypes.data, oc.ctypes.data)
                assert np.array_equal(ox[:nseg], wx) and np.array_equal(oc[:nseg], wc), \
                    (c0, cs, cnt0, n, R, "general")
                if cs >= 2.0 ** -16:
                    ox[:] = np.nan
                    oc[:] = 0
                    W.wc_code_seg_bf(c0, cs, cnt0, n, R, nseg, nseg, ox.ctypes.data,
                                     oc.ctypes.data)
                    assert np.array_equal(ox[:nseg], wx) and np.array_equal(oc[:nseg], wc), \
                        (c0, cs, cnt0, n, R, "bf")


@pytest.mark.parametrize("name", FAM)
def test_checkpoints_equal_the_planner(name):
    """checkpoints() (brute force) against G.carr_advance_ck (the host planner's walk)"""
    (blk, nch, _), lens = X.family(name)
    for n in lens:
        ck = X.checkpoints(blk, nch, n)
        for b in range(len(nch)):
            for k in range(nch[b]):
                x0, s = float(blk[b, k]["carr0"]), float(blk[b, k]["carr_step"])
                end, pk = G.carr_advance_ck(x0, s, n)
                assert np.array_equal(pk.view(np.uint64), ck[b, k].view(np.uint64)), (b, k, n)
                assert end == oracle.carr_brute(x0, s, n), (b, k, n)
            assert not ck[b, nch[b]:].any()


@pytest.mark.parametrize("case", X.OVERRUN_CASES, ids=[c[0] for c in X.OVERRUN_CASES])
def test_overrun_cases_are_what_they_say(case):
    """the oracle's rc of every overrun case: GSS_E_RANGE exactly when the wrap into word 60
    falls on one of the block's n adds, the add of the last sample included (the reference counts
    the wrap in the sample that makes it, gpssim.c:2212-2237)"""
    name, n, w, fmts = case
    blk, nch, nav = X.overrun_rows(w)
    ca = G.ca_table()
    for fmt in fmts:
        _, rc = oracle.synth(blk, nch, ca, nav, n, fmt)
        assert rc == X.overrun_expect(n, w), (name, fmt)
    # the row alone wraps on the add of sample w and not before
    p = blk[1, 2]
    st = (int(p["icode"]), int(p["ibit"]), int(p["iword"]))
    assert oracle.code_brute(float(p["code0"]), 0.25, w, *st)[1:] == st
    assert oracle.code_brute(float(p["code0"]), 0.25, w + 1, *st)[1:] == (0, 0, 60)
    # the other rows of the call never leave the nav table
    q = blk.copy()
    q[1, 2] = q[1, 1]
    assert oracle.synth(q, nch, ca, nav, n, fmts[0])[1] == 0


def test_the_issue_pair():
    """code0 = 1022.5, step 0.25, counters 19 / 29 / 59: rc -8 at n = 2 and 0 at n = 1"""
    blk, nch, nav = X.overrun_rows(1)
    assert blk[1, 2]["code0"] == 1022.5
    ca = G.ca_table()
    assert oracle.synth(blk, nch, ca, nav, 2, 16)[1] == X.E_RANGE
    assert oracle.synth(blk, nch, ca, nav, 1, 16)[1] == 0


def test_overrun_blocks_are_never_certified():
    """the fast kernel reports no status, so the proof must leave a block that runs past word 59
    to the exact path"""
    for name, n, w, _ in X.OVERRUN_CASES:
        if n % 4:
            continue
        blk, nch, nav = X.overrun_rows(w)
        _, fast = G.linearize(blk, nch, nav, n)
        if w < n:
            assert fast[1] == 0, name


def test_sum_rows_reach_the_extremes():
    """the oracle's own SC16 samples of the sum rows: I and Q reach +-(8000 * 250 + 64) >> 7 and
    take all four sign pairs, so the GPU cases are the extremes they claim to be"""
    blk, nch, nav = X.sum_rows(False)
    out, rc = oracle.synth(blk, nch, G.ca_table(), nav, X.SUM_N, 16)
    iq = out.view(np.int16).astype(np.int64)
    assert rc == 0 and iq.max() == (8000 * 250 + 64) >> 7 and iq.min() == (-8000 * 250 + 64) >> 7
    signs = {(int(np.sign(i)), int(np.sign(q))) for i, q in iq.reshape(-1, 2)}
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1)} <= signs


def test_families_reach_the_cases_meant():
    """the window period P = floor(29 / ks_max) of the rate cases, and the sums' limits"""
    def period(ks):
        return 65536 if ks < 29.0 / 65536.0 else max(1, int(29.0 / ks))
    got = [period(s) for s in X.CODE_STEPS]
    assert got[0] == 65536 and got[1] == 65536 and got[-4:] == [1, 1, 1, 1]
    assert period(14.5) == 2 and period(1.0) == 29 and period(0.9999) == 29
    for one_big, total in ((False, 8000), (True, 8001)):
        blk, nch, _ = X.sum_rows(one_big)
        assert all(int(np.abs(blk[b, :8]["gain"]).sum()) == total for b in range(len(nch)))
    for nchp in range(1, 17):
        assert max(X.instance_nch(nchp)) == nchp
