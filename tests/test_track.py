"""Signal tracking and LNAV decoding on the host (csrc/host/track.c, navdec.c):
gss_track_host against the numpy restatement of tests/trk_oracle.py, bit for bit, on random
samples where the loops never lock, and on the input families of trk_oracle.py (every epoch
length at which the kernel takes another path, saturating input, the feedback at the ends of its
arguments, jobs that end where the samples do, the longest epoch the limits admit), with the
assertions that those inputs reach what they are for; the default gains and the argument limits; the decoder on
synthetic record streams; and the physical test: the static scenario's satellites are tracked
for 12.4 s through noise, and the subframes read back are the nav rows' words at the samples the
channel rows say."""
import subprocess

import numpy as np
import pytest

import gpssim_amd as G
import acq_oracle as A
import trk_oracle as O


@pytest.mark.parametrize("fmt", [16, 8, 1])
@pytest.mark.parametrize("si", range(len(O.SHAPES)))
def test_host_equals_oracle(si, fmt):
    fs, N, n_pull, jobs = O.SHAPES[si]
    data, wrec, wcount = O.want(si, fmt, 10 * si + fmt)
    assert wcount[0] == jobs[0][3] and wcount[1] == jobs[1][3] and 0 < wcount[2] < jobs[2][3]
    assert n_pull < wcount[0]
    rec, count = G.track_host(O.trk_of(fs, fmt, O.gains_of(fs, n_pull)), data,
                              O.jobs_array(jobs), n=N, threads=2)
    O.same_records(rec, count, wrec, wcount)


def host_equals(c):
    rec, count = G.track_host(O.trk_of(c["fs"], c["fmt"], c["gains"]), c["data"],
                              O.jobs_array(c["jobs"]), n=c["N"], pitch=c["pitch"], threads=2)
    O.same_records(rec, count, c["rec"], c["count"])
    for j, n in enumerate(count):                            # rec starts zeroed
        assert not rec[j, n:].view(np.uint8).any(), j


@pytest.mark.parametrize("name", O.RATES)
def test_host_at_every_length(name):
    c = O.case(name)
    assert c["count"][0] == c["jobs"][0][3] and c["count"][1] == c["jobs"][1][3]
    assert 0 < c["count"][2] < c["jobs"][2][3]
    assert c["gains"][0] < c["count"][0]
    host_equals(c)


def seen(fs_list):
    """the epoch lengths that some job of the RATES rows of these rates runs"""
    out = set()
    for fs in fs_list:
        for fmt in (16, 8, 1):
            c = O.case(f"rate_{fs}_sc{fmt:02d}")
            for j in range(len(c["jobs"])):
                out |= set(int(n) for n in O.lengths(c, j))
    return out


def test_the_rates_reach_the_edges():
    """the lengths that matter, so that a change of the kernel's constants cannot move its
    edges away from the tests without this failing"""
    assert seen([1001]) == {1, 2}
    assert seen([2046]) == {2, 3}
    assert {63, 64} <= seen([63000]) and {64, 65} <= seen([65000])
    assert {511, 512} <= seen([511000]) and {511, 512, 513} <= seen([512000])
    assert 513 in seen([513000])
    assert {1023, 1024} <= seen([1023000])
    assert {O.AHEAD - 1, O.AHEAD} <= seen([3071000])
    assert {O.AHEAD - 1, O.AHEAD, O.AHEAD + 1} <= seen([3072000])
    assert {O.AHEAD + 1, O.AHEAD + 2} <= seen([3073000])
    # at AHEAD + 512 the next sample lands on a pass's second slot, one more and it is live
    assert {O.AHEAD + 511, O.AHEAD + 512, O.AHEAD + 513} <= seen([3584000])
    # the first pass of four samples a lane ends at AHEAD + 2048
    assert {O.AHEAD + 2048, O.AHEAD + 2049} <= seen([5120000])
    assert {O.AHEAD + 2048, O.AHEAD + 2049, O.AHEAD + 2050} <= seen([5121000])
    assert {O.FIRST_FLUSH, O.FIRST_FLUSH + 1} <= seen([64512000])
    for fs in (64512000, 64513000, 130000000):
        assert max(seen([fs])) > O.FIRST_FLUSH
    assert min(seen([130000000])) > 2 * O.FIRST_FLUSH


@pytest.mark.parametrize("name", O.SATURATING)
def test_host_saturating(name):
    c = O.case(name)
    assert c["count"][0] == 3
    sums, ymax = O.lane_sums(c)
    print(name, "largest lane sum", np.abs(sums).max(), "= 2^31 x", np.abs(sums).max() / 2**31,
          "max |y|", ymax)
    # an int32 partial sum that is never flushed overflows
    assert (sums < -2**31).any() if name.endswith("inverted") else (sums >= 2**31).any()
    host_equals(c)


@pytest.mark.parametrize("name", O.FEEDBACK)
def test_host_feedback(name):
    c = O.case(name)
    kind = name.rsplit("_", 1)[1]
    assert (c["count"] > 10).all()
    if kind == "pullall":
        assert c["gains"][0] > max(j[3] for j in c["jobs"])
    if kind == "wrap":                                       # w changes sign by wrapping
        w = c["rec"]["w"].astype(np.int64)
        assert any((np.abs(np.diff(w[j, :n])) > 2**31).any() for j, n in enumerate(c["count"]))
    if kind == "maxkd":                                      # the length hint falls back
        assert max(np.abs(np.diff(O.lengths(c, j))).max() for j in range(3)) > 1
    if kind == "zeros":
        # every discriminator takes its 0 / 0 branch
        assert not c["rec"]["IP"].any() and not c["rec"]["IL"].any()
        assert all((c["rec"]["w"][j] == job[2]).all() for j, job in enumerate(c["jobs"]))
    host_equals(c)


@pytest.mark.parametrize("name", O.ENDS)
def test_host_ends(name):
    c = O.case(name)
    kind = name.split("_", 2)[2]
    if kind in ("exact", "short"):
        assert list(c["count"]) == [40 if kind == "exact" else 39, 0, 0, 0, 0, 1, 10]
        end = c["rec"]["s"][0, 39] if kind == "short" else None
        assert end is None or end < c["N"]
    else:
        k = int(kind[-1])
        assert c["N"] % 4 == (O.case(name[:-1] + "0")["N"] - k) % 4
        assert sorted(j[1] % 4 for j in c["jobs"]) == [0, 1, 2, 3]
        assert c["count"][0] == (40 if k == 0 else 39) and (c["count"] >= 38).all()
    assert c["pitch"] > max(j[3] for j in c["jobs"])
    host_equals(c)


def test_host_longest_epoch():
    """2 GS/s, w0 = -2^31, the largest Kd the limits admit and an input that drives the code
    step to its floor: the second epoch is nearly 2^23 samples, and its length stays an int32"""
    c = O.case(O.LONGEST)
    assert c["count"][0] == 2
    cs1 = O.cs_nominal(c["fs"]) + int(c["rec"]["dcs"][0, 1])
    n1 = -(-(O.M - (int(O.lengths(c, 0)[0]) * (O.cs_nominal(c["fs"]) + int(c["rec"]["dcs"][0, 0]))
                   - O.M)) // cs1)
    print("code step", cs1, "floor", O.CS_MIN + 1, "epoch", n1, "of 2^23 =", 2**23)
    assert O.CS_MIN < cs1 < O.CS_MIN + 1200 and 8370000 < n1 < 2**23
    host_equals(c)


def test_default_gains():
    for fs, want in ((1000000, (3161, 131452, 136713, 68719)),
                     (2600000, (1216, 50559, 52582, 26431))):
        t = G.Trk(fs, 16)
        assert (t.Ki, t.Kp, t.Kf, t.Kd) == want and t.n_pull == 300 and t.fs_hz == fs
        assert O.defaults(fs) == (300, want[2], want[0], want[1], want[3])
    assert O.cs_nominal(1000000) == round(1023000 * 2**32 / 1000000)


def test_job_from_peak():
    acq = G.Acq(1000000, 16, 1, 10, 250, 20)
    pk = np.zeros(2, G.ACQ_PEAK_DTYPE)
    pk[0] = (1, 1, 1, 417, -7, 23)
    pk[1] = (1, 1, 1, 0, 12, 1)
    jobs = G.trk_jobs(acq, pk, 5000, 77)
    assert [tuple(j) for j in jobs] == [
        (5417, 23, O.s32((-7 * 250 * 2**32 + 500000) // 1000000), 77, 0),
        (5000, 1, (12 * 250 * 2**32 + 500000) // 1000000, 77, 0)]


def test_argument_limits():
    fs = 64000
    x = O.random_samples(1000, 16, 1)
    ok = O.jobs_array([(1, 0, 0, 4)])

    def bad(trk, jobs, **kw):
        with pytest.raises(G.GssError) as e:
            G.track_host(trk, x, jobs, **kw)
        assert e.value.code == -1

    G.track_host(G.Trk(fs, 16), x, ok)
    for prn in (0, 33, -1):
        bad(G.Trk(fs, 16), O.jobs_array([(prn, 0, 0, 4)]))
    bad(G.Trk(fs, 16), O.jobs_array([(1, -1, 0, 4)]))
    bad(G.Trk(fs, 16), O.jobs_array([(1, 0, 0, -1)]))
    # s0 so large that s0 + an epoch would leave int64 (the sum used to wrap to a sample in
    # front of the buffer); 2^62 itself is far behind N: no epoch
    bad(G.Trk(fs, 16), O.jobs_array([(1, 2**63 - 1, 0, 4)]))
    bad(G.Trk(fs, 16), O.jobs_array([(1, 2**62 + 1, 0, 4)]))
    assert G.track_host(G.Trk(fs, 16), x, O.jobs_array([(1, 2**62, 0, 4)]))[1][0] == 0
    bad(G.Trk(fs, 16), ok, pitch=3)                          # n_epoch above pitch
    bad(G.Trk(fs, 16, Kd=-1), ok)
    bad(G.Trk(fs, 16, Kp=2**30 + 1), ok)
    bad(G.Trk(fs, 16, n_pull=-1), ok)
    t = G.Trk(fs, 16)
    t.fmt = 4
    bad(t, ok)
    # the code step could reach a whole period (fs so low that cs_nom + the span >= M) or 0
    t.fmt = 16
    t.fs_hz = 1000
    bad(t, ok)
    with pytest.raises(G.GssError):
        G.Trk(999, 16)
    t = G.Trk(2000000000, 16)                                # cs_nom 2.2e6 > span 1.39e6: accepted
    t.Kd = 2**30                                             # span + Kd / 4 > cs_nom
    bad(t, ok)
    # The code step could fall to M >> 23, an epoch reach 2^23 samples.  Kd = 3,209,600 leaves
    # cs_nom - span = 3: with w0 = -2^31 and an input that empties the early correlator the
    # second epoch would need 2.8e9 samples, more than its int32 length holds.  Rejected before
    # anything runs (and never to be run un-rejected).
    kw = dict(n_pull=0, Kf=0, Ki=0, Kp=0)
    far = O.jobs_array([(1, 0, -2**31, 4)])
    x8 = O.random_samples(1000, 8, 2)
    assert O.cs_nominal(2000000000) - (O.WSPAN + 3209600 // 4 + 2) == 3
    with pytest.raises(G.GssError) as e:
        G.track_host(G.Trk(2000000000, 8, Kd=3209600, **kw), x8, far)
    assert e.value.code == -1 and "2^23" in str(e.value)
    fs, inside, outside = O.longest_cfg()
    with pytest.raises(G.GssError) as e:
        G.track_host(O.trk_of(fs, 8, outside), x8, far)
    assert e.value.code == -1
    rec, count = G.track_host(O.trk_of(fs, 8, inside), x8, far)   # accepted: no epoch fits
    assert count[0] == 0
    for f in (16, 8, 1):                                      # what the suite tracks stays accepted
        for r in [s[0] for s in O.SHAPES] + [r for r, _ in O.RATE_TABLE] + [1000000, 2000000000]:
            G.track_host(G.Trk(r, f), x, O.jobs_array([(1, 10**6, 0, 1)]))
    # SC16 samples at an odd address
    raw = np.zeros(4001, np.uint8)
    with pytest.raises(G.GssError):
        G.track_host(G.Trk(fs, 16), raw[1:], ok, n=1000)


# ---- the decoder on synthetic record streams -----------------------------------------------
def nav_row():
    """a nav-table row of the static scenario: six subframes' worth of words with parity"""
    from conftest import LOC, NAV
    s = G.Scenario(NAV, llh=LOC, duration=0.1, samp_freq=1e6)
    s.next(1)
    row = s.nav_table()[0].copy()
    s.close()
    return row


def stream(row, offset, invert, lead_bits=3, skip=500, flip=None):
    """records whose IP carries the row's 1800 bits, 20 epochs each, +-1000: the first bit
    starts at epoch skip + offset + 20 lead_bits behind filler bits; flip: a bit to invert"""
    bits = np.array([(int(w) >> (29 - i)) & 1 for w in row for i in range(30)], np.int64)
    if flip is not None:
        bits[flip] ^= 1
    lead = np.resize(np.array([1, 0, 0, 1, 1, 0, 1], np.int64), lead_bits)
    allbits = np.concatenate([lead, bits, lead])
    ip = np.repeat(2 * allbits - 1, 20) * 1000
    # in front of the first bit: the tail of a bit that ends where the offset says
    head = np.full(skip + offset, 1000, np.int64)
    head[:skip] = np.resize(np.repeat(np.array([1, -1], np.int64) * 1000, 20), skip)
    ip = np.concatenate([head, ip])
    rec = np.zeros(len(ip), G.TRK_REC_DTYPE)
    rec["IP"] = -ip if invert else ip
    rec["s"] = 1000 * np.arange(len(ip)) + 123
    return rec, skip + offset + 20 * lead_bits


@pytest.fixture(scope="module")
def row():
    return nav_row()


@pytest.mark.parametrize("invert", [False, True])
def test_decoder_every_offset(row, invert):
    for offset in range(20):
        rec, first = stream(row, offset, invert)
        sfs, off = G.nav_decode(rec)
        assert off == offset
        assert len(sfs) == 6
        for k, sf in enumerate(sfs):
            assert np.array_equal(sf["word"], row[10 * k:10 * k + 10])
            assert sf["epoch"] == first + 6000 * k and sf["sample"] == 1000 * sf["epoch"] + 123
            assert sf["polarity"] == int(invert)
            how = int(row[10 * k + 1]) ^ (0x3FFFFFC0 if int(row[10 * k]) & 1 else 0)
            assert sf["tow"] == (how >> 13) & 0x1FFFF and sf["id"] == (how >> 8) & 7
        assert [int(sf["id"]) for sf in sfs[1:]] == [1, 2, 3, 4, 5]
        assert np.array_equal(np.diff(sfs["tow"][1:]), [1, 1, 1, 1])


def test_decoder_one_flipped_bit(row):
    rec, first = stream(row, 7, False, flip=300 * 2 + 30 * 4 + 11)     # subframe 2, word 4
    sfs, off = G.nav_decode(rec)
    assert off == 7
    assert [int(sf["epoch"]) for sf in sfs] == [first + 6000 * k for k in (0, 1, 3, 4, 5)]
    for sf, k in zip(sfs, (0, 1, 3, 4, 5)):
        assert np.array_equal(sf["word"], row[10 * k:10 * k + 10])


def test_decoder_short_and_bad_input(row):
    rec, _ = stream(row, 0, False)
    assert len(G.nav_decode(rec[:530])[0]) == 0              # fewer than two bits behind skip
    assert len(G.nav_decode(rec[:3000])[0]) == 0             # no whole subframe
    assert len(G.nav_decode(rec, cap=2)[0]) == 2
    assert G.lib().gss_nav_decode(None, 10, -1, None, 0, None) == -1


def test_cn0_by_moments():
    """a constant prompt amplitude A in complex Gaussian noise of variance 2 s^2 per epoch reads
    10 log10(A^2 / (2 s^2) / 1 ms)"""
    rng = np.random.default_rng(3)
    n, amp, s = 20000, 40000.0, 4000.0
    rec = np.zeros(n, G.TRK_REC_DTYPE)
    rec["IP"] = np.rint(amp * np.where(rng.integers(0, 2, n) == 1, 1, -1)
                        + s * rng.standard_normal(n)).astype(np.int64)
    rec["QP"] = np.rint(s * rng.standard_normal(n)).astype(np.int64)
    want = 10 * np.log10(amp**2 / (2 * s**2) / 1e-3)
    assert abs(G.trk_cn0(rec, 0) - want) < 0.2
    assert np.isnan(G.trk_cn0(rec[:1], 0))
    rec["IP"], rec["QP"] = 1000, 0                           # no noise at all: Pn == 0
    assert np.isnan(G.trk_cn0(rec, 0))


# ---- the physical test -----------------------------------------------------------------------
def tracked(fmt, clean=False):
    data = O.phys_samples(fmt, clean)
    peaks, _, _ = G.acquire_host(O.phys_acq(fmt), data)
    jobs, keep = O.phys_jobs(fmt, peaks)
    assert len(jobs) == len(keep) >= 8
    rec, count = G.track_host(G.Trk(A.PHYS_FS, fmt), data, jobs, threads=8)
    return rec, count, jobs, keep


@pytest.mark.parametrize("fmt", [16, 8])
def test_physical_with_level(fmt):
    rec, count, jobs, keep = tracked(fmt)
    O.check_decode(rec, count, jobs, keep, level=O.LEVEL)


def test_physical_one_bit():
    rec, count, jobs, keep = tracked(1)
    O.check_decode(rec, count, jobs, keep)


def test_physical_noise_free_has_no_bit_errors():
    rec, count, jobs, keep = tracked(16, clean=True)
    O.check_decode(rec, count, jobs, keep, want_sf=1, every_bit=True)


def test_tool_on_the_host(tmp_path):
    """gps-sdr-track --host on the physical file: the steady PRNs with their subframes"""
    data = O.phys_samples(16)
    f, r = tmp_path / "phys.bin", tmp_path / "rec.bin"
    data.tofile(f)
    rec, count, jobs, keep = tracked(16)
    prns = ",".join(str(p) for p in sorted(keep))
    out = subprocess.run([G.TRK_CLI_PATH, "-f", str(f), "-s", str(A.PHYS_FS), "-b", "16",
                          f"--prn={prns}", "--host", f"--records={r}"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head = [ln.split() for ln in lines if ln.startswith("PRN")]
    assert [int(h[1]) for h in head] == sorted(keep)
    got = np.fromfile(r, G.TRK_REC_DTYPE)
    ne = int(head[0][5])
    assert all(int(h[5]) == ne and int(h[7]) == 1 for h in head) and len(got) == ne * len(head)
    # the tool's search spans +-5 kHz where the test's spans +-5 kHz too: the same jobs, so its
    # first PHYS_EPOCHS records are the test's
    for j in range(len(head)):
        assert np.array_equal(got[j * ne:j * ne + O.PHYS_EPOCHS], rec[j, :O.PHYS_EPOCHS])
    for j, h in enumerate(head):
        prn = int(h[1])
        sfs, off = G.nav_decode(got[j * ne:(j + 1) * ne])
        assert int(h[13]) == off and int(h[15]) == len(sfs) >= 1
        mine = [ln.split() for ln in lines if ln.startswith(f"SF {prn:2d} ")]
        assert [(int(m[5]), int(m[7]), int(m[9])) for m in mine] == [
            (int(s["sample"]), int(s["tow"]), int(s["id"])) for s in sfs]
    usage = subprocess.run([G.TRK_CLI_PATH], capture_output=True, text=True)
    assert usage.returncode == 1 and "straddles" in usage.stderr

