"""The acquisition search on the host (csrc/host/acquire.c, csrc/common/gss_acq.h): exactness
against the numpy restatement of tests/acq_oracle.py, the argument limits, the threshold's
defining equation, and the physical test: the satellites of a rendered block are found where the
channel rows say, at the level the noise option asked for."""
import subprocess

import numpy as np
import pytest

import gpssim_amd as G
import acq_oracle as O
from acq_oracle import SHAPES, random_samples


def acq_of(shape, fmt=16, qshift=-1):
    fs, coh, M, K, df, prns = shape
    return G.Acq(fs, fmt, coh, M, df, K, qshift, prns)


def check_exact(shape, fmt, data, qshift):
    fs, coh, M, K, df, prns = shape
    want_p, want_g, want_sh = O.acquire(data, fs, fmt, coh, M, K, df, prns, qshift)
    peaks, grid, sh = G.acquire_host(acq_of(shape, fmt, qshift), data, want_grid=True)
    assert sh == want_sh
    assert np.array_equal(grid, want_g)
    assert np.array_equal(peaks, want_p), (peaks, want_p)
    nogrid, none, sh2 = G.acquire_host(acq_of(shape, fmt, qshift), data)
    assert none is None and sh2 == sh and np.array_equal(nogrid, want_p)


@pytest.mark.parametrize("qshift", [0, 7, -1])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_host_equals_oracle_sc16(si, qshift):
    """full-range random int16: with shift 0 and 7 the clamp fires"""
    s = SHAPES[si]
    check_exact(s, 16, random_samples(s[0], s[1], s[2], 16, seed=si + 1), qshift)


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_host_equals_oracle_extreme(si):
    """every component at +32767 / -32768: the largest sums"""
    s = SHAPES[si]
    data = random_samples(s[0], s[1], s[2], 16, seed=50 + si, extreme=True)
    check_exact(s, 16, data, -1)
    if si < 2:
        check_exact(s, 16, data, 17)


@pytest.mark.parametrize("fmt", [8, 1])
@pytest.mark.parametrize("si", [0, 1])
def test_host_equals_oracle_sc08_sc01(si, fmt):
    s = SHAPES[si]
    data = random_samples(s[0], s[1], s[2], fmt, seed=20 + si)
    for qshift in (-1, 0):
        check_exact(s, fmt, data, qshift)


@pytest.mark.parametrize("si", [0, 1])
def test_host_odd_sample_start(si):
    """the sample pointer one and three samples (and, SC08, one byte pair) into a buffer"""
    s = SHAPES[si]
    fs, coh, M = s[:3]
    N = O.sizes(fs, coh, M)[2]
    rng = np.random.default_rng(9)
    buf = rng.integers(-32768, 32768, 2 * (N + 3)).astype("<i2")
    for off in (1, 3):
        check_exact(s, 16, buf[2 * off:].view(np.uint8), 5)
    b8 = rng.integers(-128, 128, 2 * (N + 1)).astype(np.int8)
    check_exact(s, 8, b8[2:].view(np.uint8), -1)


def test_ties_take_the_lowest_bin_then_tau():
    """all-zero samples: every cell ties at 0, the peak is bin -K, tau 0"""
    s = SHAPES[0]
    peaks, _, _ = G.acquire_host(acq_of(s, 16, 0), np.zeros(4 * O.sizes(*s[:3])[2], np.uint8))
    assert (peaks["tau"] == 0).all() and (peaks["bin"] == -s[3]).all()
    assert (peaks["peak"] == 0).all() and (peaks["floor_sum"] == 0).all()


def check_case(case):
    """gss_acquire_host over a case of acq_oracle against the oracle's shared answer (which
    holds the case's precondition), with and without the grid"""
    _, shape, fmt, _, qshift = case
    want_p, want_g, want_sh = O.answer(case)
    data = O.case_data(case)
    peaks, grid, sh = G.acquire_host(acq_of(shape, fmt, qshift), data, want_grid=True)
    assert sh == want_sh
    assert np.array_equal(grid, want_g), np.argwhere(grid != want_g)[:8]
    assert np.array_equal(peaks, want_p), (peaks, want_p)
    nogrid, none, sh2 = G.acquire_host(acq_of(shape, fmt, qshift), data)
    assert none is None and sh2 == sh and np.array_equal(nogrid, want_p)


EDGE_CASES = O.edge_cases()


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_host_equals_oracle_edge_shapes(case):
    """window lengths that are no multiple of 4, exact and just-exceeded tau tiles and chunks,
    16 and 17 PRNs, one bin and 261 bins, the largest n_coh: every format and shift"""
    check_case(case)


@pytest.mark.parametrize("case", O.SPECIAL_CASES, ids=[c[0] for c in O.SPECIAL_CASES])
def test_host_planted_peaks_and_ties(case):
    """peaks planted at both ends of the code period (the floor's zone wraps), and inputs whose
    cells tie at a non-zero value across bins, across a pair of bins and along a whole row: the
    lowest bin, then the lowest code phase"""
    check_case(case)


def test_argument_errors():
    ok = dict(fs_hz=1000000, fmt=16, coh_ms=1, n_coh=2, bin_hz=500, n_half=2, qshift=-1)
    x = np.zeros(8 * 4000, np.uint8)
    G.acquire_host(G.Acq(**ok, prns=[1]), x)
    bad = [dict(coh_ms=2, fs_hz=600000000),       # L = 1.2e6 > 2^20
           dict(n_coh=1001), dict(n_coh=0), dict(coh_ms=0), dict(bin_hz=0), dict(n_half=-1),
           dict(fs_hz=4000),                      # T = 4 <= 2 E + 1 = 5
           dict(fmt=4), dict(qshift=25), dict(qshift=-2)]
    for b in bad:
        with pytest.raises(G.GssError) as e:
            G.acquire_host(G.Acq(**{**ok, **b}, prns=[1]), x)
        assert e.value.code == -1, b
        with pytest.raises(G.GssError) as e:
            G.Acq(**{**ok, **b}).sizes()
        assert e.value.code == -1, b
    with pytest.raises(G.GssError) as e:
        G.acquire_host(G.Acq(**ok, prns=[]), x)
    assert e.value.code == -1
    odd = np.zeros(8 * 4000 + 2, np.uint8)[1:]    # SC16 at an odd address
    with pytest.raises(G.GssError) as e:
        G.acquire_host(G.Acq(**ok, prns=[1]), odd)
    assert e.value.code == -1


def test_doppler_holes_warn_only():
    a = G.Acq(1000000, 16, 2, 1, 500, 1, -1, [1])
    a.sizes()
    assert "Doppler holes" in G.lib().gss_last_error().decode()


@pytest.mark.parametrize("M", [1, 8, 20])
def test_threshold_satisfies_its_equation(M):
    for cells, pfa in ((21000, 1e-3), (1, 0.5), (41 * 2600, 1e-6)):
        r = G.acq_threshold(M, cells, pfa)
        assert abs(O.threshold_equation(M, r * M) / (pfa / cells) - 1) <= 1e-9, (M, cells, pfa)
    assert np.isnan(G.acq_threshold(0, 10, 1e-3)) and np.isnan(G.acq_threshold(1, 10, 0.0))


def test_expect_labels():
    row = np.zeros(1, G.CHAN_DTYPE)[0]
    row["code0"], row["code_step"], row["carr_step"] = 1000.0, 1.023, -0.0025
    row["gain"], row["ca_tbl"] = 64, 16
    t = G.acq_expect(row, 1e6, 0)
    assert t["prn"] == 17 and abs(t["tau"] - 23 / 1.023) < 1e-9
    assert abs(t["doppler_hz"] + 2500) < 1e-9 and abs(t["cn0_offset_db"] + 6.0206) < 1e-4
    t = G.acq_expect(row, 1e6, 100)                # 102.3 chips later: the period wraps
    assert abs(t["tau"] - ((23 - 102.3) / 1.023 + 1000)) < 1e-6


# ---- physical --------------------------------------------------------------------------------
def test_physical_sc16(noisy):
    data, blk, nch = noisy(16)
    peaks, _, sh = G.acquire_host(O.PHYS_ACQ(16), data)
    O.check_physical(peaks, blk, nch, level=True)


def test_physical_sc08(noisy):
    data, blk, nch = noisy(8)
    peaks, _, sh = G.acquire_host(O.PHYS_ACQ(8), data)
    O.check_physical(peaks, blk, nch, level=True)


def test_physical_sc01(noisy):
    data, blk, nch = noisy(1)
    peaks, _, _ = G.acquire_host(O.PHYS_ACQ(1), data)
    O.check_physical(peaks, blk, nch, level=False, found=False)     # location only


def test_noise_free_block_is_located(noisy):
    data, blk, nch = noisy(16, clean=True)
    peaks, _, _ = G.acquire_host(G.Acq(O.PHYS_FS, 16, 1, 2, 500, 10, -1), data)
    O.check_physical(peaks, blk, nch, level=False, found=False)


def test_cli_host(noisy, tmp_path):
    data, blk, nch = noisy(16)
    f = tmp_path / "noisy.bin"
    data.tofile(f)
    p = subprocess.run([G.ACQ_CLI_PATH, "-f", str(f), "-s", str(O.PHYS_FS), "-b", "16", "--host",
                        "--ncoh=8", "--fmax=5000"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = [ln.split() for ln in p.stdout.splitlines()]
    peaks, _, _ = G.acquire_host(O.PHYS_ACQ(16), data)
    thr = O.phys_threshold()
    assert len(rows) == 32
    for r, pk in zip(rows, peaks):
        assert (int(r[0]), int(r[2]), int(r[3])) == (pk["prn"], pk["tau"], pk["bin"] * 500)
        assert int(r[1]) == int(G.acq_ratio(pk) >= thr)
        assert abs(float(r[4]) - G.acq_ratio(pk)) < 1e-5
        assert abs(float(r[5]) - G.cn0_dbhz(pk)) < 2e-3


def test_cli_usage_errors(tmp_path):
    f = tmp_path / "short.bin"
    f.write_bytes(b"\0" * 100)
    for args in ([], ["-f", str(f)], ["-f", str(f), "-s", "1e6", "-b", "4"],
                 ["-f", str(f), "-s", "1e6", "--prn=0"], ["-f", str(f), "-s", "1e6", "--bogus"],
                 ["-f", str(f), "-s", "1e6", "--host"],          # the file is too short
                 ["-f", str(tmp_path / "none.bin"), "-s", "1e6", "--host"]):
        p = subprocess.run([G.ACQ_CLI_PATH] + args, capture_output=True, text=True)
        assert p.returncode == 1 and p.stderr and not p.stdout, args


@pytest.fixture(scope="module")
def noisy():
    return O.noisy_block
