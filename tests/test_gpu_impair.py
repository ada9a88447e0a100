"""Additive noise on the GPU (csrc/hip/gss_impair.hip, gss_run with gss_run_opts_t.impair, the
CLI's --cn0 / --noise-sigma / --noise-shift / --seed): every byte against the numpy restatement
of tests/impair_oracle.py applied to the noise-free SC16 samples, which the existing parity tests
pin to the reference."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import impair_oracle as O
from impair_oracle import SHIFTS, SIGMAS, SIZES, STARTS, samples

pytestmark = pytest.mark.gpu

SEED = 7
LOC_ARG = "%.6f,%.6f,%g" % LOC


def sigma_cn0(fs, cn0=45.0):
    return int(np.floor(256 * 250 * np.sqrt(fs / (2 * 10 ** (cn0 / 10))) + 0.5))


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


def on_device(dev, imp, iq, s0, fmt, in_off=0, out_off=0, in_place=False):
    """gss_impair_device over iq (host int16[2 n]) placed in_off samples into a device buffer,
    the output out_off bytes into another (or the input's place); returns the bytes"""
    import torch
    n = len(iq) // 2
    nb = G.impair_bytes(n, fmt)
    d_in = torch.zeros(2 * (n + in_off) + 8, dtype=torch.int16, device="cuda")
    d_in[2 * in_off:2 * (in_off + n)] = torch.from_numpy(iq).cuda()
    guard = 64
    d_out = torch.full((nb + out_off + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    p_in = d_in.data_ptr() + 4 * in_off
    p_out = p_in if in_place else d_out.data_ptr() + out_off
    dev.impair_device(imp, p_in, s0, n, fmt, p_out)
    torch.cuda.synchronize()
    if in_place:
        return d_in[2 * in_off:2 * (in_off + n)].cpu().numpy().view(np.uint8)
    got = d_out.cpu().numpy()
    assert (got[:out_off] == 0xA5).all() and (got[out_off + nb:] == 0xA5).all(), "wrote outside"
    return got[out_off:out_off + nb]


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_impair_device_equals_oracle(dev, fmt):
    for n in SIZES[fmt]:
        iq = samples(n, seed=n)
        for sigma in SIGMAS:
            for shift in SHIFTS:
                for s0 in STARTS:
                    seed = (0x9E3779B97F4A7C15 * (s0 + 1) + sigma) & (2**64 - 1)
                    got = on_device(dev, G.Impair(sigma, shift, seed), iq, s0, fmt)
                    want = O.impair(seed, sigma, shift, iq, s0, fmt)
                    assert np.array_equal(got, want), (fmt, n, sigma, shift, s0)


@pytest.mark.parametrize("s0", [0, 1, 2**32 - 5])
def test_impair_device_in_place_sc16(dev, s0):
    for n in SIZES[16]:
        iq = samples(n, seed=3)
        for off in (0, 3):
            got = on_device(dev, G.Impair(256 * 994, 0, SEED), iq, s0, 16, in_off=off,
                            in_place=True)
            assert np.array_equal(got, O.impair(SEED, 256 * 994, 0, iq, s0, 16)), (n, off)


def test_table_lives_and_dies_with_the_handle():
    """the noise table is uploaded when a handle opens and freed when it closes: a handle opened
    after a close impairs from its own copy"""
    d = G.Device(0)
    try:
        n, sigma, shift, s0 = SIZES[1][-1], SIGMAS[2], SHIFTS[1], STARTS[1]     # SC01, odd start
        iq = samples(n, seed=n)
        seed = (0x9E3779B97F4A7C15 * (s0 + 1) + sigma) & (2**64 - 1)
        got = on_device(d, G.Impair(sigma, shift, seed), iq, s0, 1)
        assert np.array_equal(got, O.impair(seed, sigma, shift, iq, s0, 1))
    finally:
        d.close()
    d = G.Device(0)
    try:
        n, s0 = SIZES[16][-1], 2**32 - 5
        iq = samples(n, seed=3)
        got = on_device(d, G.Impair(256 * 994, 0, SEED), iq, s0, 16, in_place=True)
        assert np.array_equal(got, O.impair(SEED, 256 * 994, 0, iq, s0, 16))
    finally:
        d.close()


@pytest.mark.parametrize("fmt,in_off,out_off", [
    (16, 1, 4), (16, 3, 12), (16, 1, 8), (16, 0, 2),    # the last two never line up: edges only
    (8, 1, 2), (8, 3, 6), (8, 7, 14), (8, 1, 1),
    (1, 0, 1), (1, 0, 3), (1, 4, 0), (1, 1, 0),
])
def test_impair_device_unaligned_pointers(dev, fmt, in_off, out_off):
    """input and output at every alignment class: a head of 0..15 samples before the 16-byte
    groups, or (pointers that never line up together) every sample through the edge path"""
    n = 7804
    iq = samples(n, seed=11)
    for s0 in (0, 1):
        got = on_device(dev, G.Impair(256 * 500, 1, SEED), iq, s0, fmt, in_off, out_off)
        assert np.array_equal(got, O.impair(SEED, 256 * 500, 1, iq, s0, fmt)), s0


def test_impair_device_grid_stride(dev):
    """more groups than the capped grid has threads (2,048 x 256 x 4 samples at SC16), an odd
    start and a tail"""
    n = 2048 * 256 * 4 + 4099
    iq = samples(n, seed=5)
    s0 = 2**33 + 3
    got = on_device(dev, G.Impair(256 * 994, 0, SEED), iq, s0, 16)
    assert np.array_equal(got, O.impair(SEED, 256 * 994, 0, iq, s0, 16))


def test_impair_device_argument_errors(dev):
    import torch
    d_in = torch.zeros(64, dtype=torch.int16, device="cuda")
    d_out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    pi, po = d_in.data_ptr(), d_out.data_ptr()
    for imp, n, fmt, out in [(G.Impair(0x1000000, 0, 0), 8, 16, po), (G.Impair(1, 9, 0), 8, 16, po),
                             (G.Impair(1, 0, 0), 8, 4, po), (G.Impair(1, 0, 0), 6, 1, po),
                             (G.Impair(1, 0, 0), 8, 8, pi), (G.Impair(1, 0, 0), 8, 1, pi),
                             (G.Impair(1, 0, 0), 8, 16, 0)]:
        with pytest.raises(G.GssError) as e:
            dev.impair_device(imp, pi, 0, n, fmt, out)
        assert e.value.code == -1
    torch.cuda.synchronize()


# ---- runs ----------------------------------------------------------------------------------------
def scenario(fs, fmt):
    return G.Scenario(NAV, llh=LOC, duration=1.0, samp_freq=fs, data_format=fmt)


def run_bytes(dev, fs, fmt, impair=None, **kw):
    s = scenario(fs, fmt)
    parts, seen = [], []

    def sink(buf, first, nb):
        parts.append(bytes(buf))
        seen.append((first, nb))

    dev.run(s, sink, impair=impair, **kw)
    n_per_blk = s.n_per_blk
    s.close()
    for (a, na), (b, _) in zip(seen, seen[1:]):
        assert a + na == b
    return np.frombuffer(b"".join(parts), np.uint8), n_per_blk, seen


_plain = {}


@pytest.fixture(scope="module")
def plain(dev):
    """fs -> (the noise-free -b 16 run's int16 samples, n_per_blk, the oracle's noise for them):
    computed once per rate, shared by every run test"""
    def get(fs):
        if fs not in _plain:
            raw, npb, _ = run_bytes(dev, fs, 16, batch=128)
            iq = raw.view(np.int16)
            assert len(iq) == 2 * 9 * npb
            assert np.abs(iq.astype(np.int32)).max() <= 2047        # the reference peaks at 1377
            _plain[fs] = (iq, npb, O.noise(SEED, sigma_cn0(fs), 0, len(iq) // 2))
        return _plain[fs]
    return get


def shift_for(fmt):
    return {16: 0, 8: 2, 1: 0}[fmt]                  # the CLI's auto shift at 45 dB-Hz


def expect(plain, fs, fmt, first=0, nblk=9):
    iq, npb, g = plain(fs)
    lo, hi = first * npb, (first + nblk) * npb
    return O.impair(SEED, sigma_cn0(fs), shift_for(fmt), iq[2 * lo:2 * hi], lo, fmt, g=g[lo:hi])


# 1000010: n_per_blk = 100001, so block starts alternate parity (and -b 1 is not defined)
CASES = [(1000000, 16), (1000000, 8), (1000000, 1), (1000010, 16), (1000010, 8)]
MODES = {
    "batch2": ({}, dict(batch=2)),
    "batch128": ({}, dict(batch=128)),
    "range": ({}, dict(batch=3, first_block=3, n_blocks=4)),
    "gpu_exact3": ({"GSS_RUN_PROOF": "gpu", "GSS_RUN_FORCE_EXACT": "3"}, dict(batch=4)),
    "gpu_exact3_late": ({"GSS_RUN_PROOF": "gpu", "GSS_RUN_FORCE_EXACT": "3",
                         "GSS_RUN_LATE_VERDICTS": "1"}, dict(batch=4)),
    "walk": ({"GSS_PATH": "walk"}, dict(batch=4)),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fs,fmt", CASES)
def test_run_with_noise_equals_oracle(dev, plain, monkeypatch, fs, fmt, mode):
    want_all = expect(plain, fs, fmt)              # (the plain run before the mode's environment)
    env, kw = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    imp = G.Impair(sigma_cn0(fs), shift_for(fmt), SEED)
    got, npb, seen = run_bytes(dev, fs, fmt, impair=imp, threads=4, **kw)
    if mode == "range":
        assert seen[0][0] == 3 and sum(nb for _, nb in seen) == 4
        bb = G.block_bytes(npb, fmt)
        assert np.array_equal(got, want_all[3 * bb:7 * bb])
        assert np.array_equal(got, expect(plain, fs, fmt, 3, 4))
    else:
        assert sum(nb for _, nb in seen) == 9
        assert np.array_equal(got, want_all)


@pytest.mark.parametrize("fs,fmt", CASES)
def test_zero_noise_is_the_plain_run(dev, fs, fmt):
    """sigma 0, shift 0 through the SC16 render and the impair kernel: the plain run's bytes"""
    want, _, _ = run_bytes(dev, fs, fmt, batch=4)
    got, _, _ = run_bytes(dev, fs, fmt, impair=G.Impair(0, 0, 123), batch=4)
    assert np.array_equal(got, want)


def test_cli_cn0(dev, golden, tmp_path):
    """--cn0=45 --seed=7 -b 8 at the default rate: the resolved sigma on stderr, within 1 of the
    formula, and the file's bytes by the oracle from it; without the options, the reference's
    bytes as before (the first blocks of the golden 30 s run)."""
    args = [G.CLI_PATH, "-e", NAV, "-l", LOC_ARG, "-d", "1", "-b", "8"]
    out = tmp_path / "noisy.bin"
    p = subprocess.run(args + ["--cn0=45", "--seed=7", "-o", str(out)], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"^Noise: sigma_q8 = (\d+), shift = (-?\d+), seed = (\d+)$", p.stderr, re.M)
    assert m, p.stderr[-2000:]
    sigma, shift, seed = map(int, m.groups())
    assert abs(sigma - sigma_cn0(2.6e6)) <= 1 and seed == 7
    assert shift == min(k for k in range(9) if 4 * sigma / 256 + 2047 <= 2047 * 2**k) == 3
    s = G.Scenario(NAV, llh=LOC, duration=1.0, data_format=16)
    parts = []
    dev.run(s, lambda buf, first, nb: parts.append(bytes(buf)), batch=128)
    bb16 = G.block_bytes(s.n_per_blk, 16)
    s.close()
    raw = b"".join(parts)
    hs = [hashlib.sha256(raw[i:i + bb16]).hexdigest()[:16] for i in range(0, len(raw), bb16)]
    assert hs == golden["static_d30_b16"]["block_sha16"][:9]
    iq = np.frombuffer(raw, np.int16)
    got = np.fromfile(out, np.uint8)
    assert np.array_equal(got, O.impair(seed, sigma, shift, iq, 0, 8))

    quiet = tmp_path / "plain.bin"
    p = subprocess.run(args + ["-o", str(quiet)], capture_output=True, text=True)
    assert p.returncode == 0 and "Noise:" not in p.stderr
    raw = open(quiet, "rb").read()
    bb8 = bb16 // 2
    hs = [hashlib.sha256(raw[i:i + bb8]).hexdigest()[:16] for i in range(0, len(raw), bb8)]
    assert hs == golden["static_d30_b8"]["block_sha16"][:9]


def test_run_node_refuses_noise_options():
    from gpssim_amd.node import run_node
    with pytest.raises(ValueError, match="noise"):
        run_node(["-e", NAV, "-l", LOC_ARG, "-d", "1", "--noise-sigma=100"], 0, 1, 0)
