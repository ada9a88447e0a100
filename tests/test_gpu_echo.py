"""Multipath echoes on the GPU (csrc/hip/gss_echo.hip, gss_run with gss_run_opts_t.echo, the
CLI's --multipath): every byte against the restatement of tests/echo_oracle.py in both forms of
the kernel, and the runs against gss_jam_host over gss_echo_host over the plain SC16 run, which
the existing parity tests pin to the reference."""
import subprocess

import numpy as np
import pytest

from conftest import LOC, NAV

import gpssim_amd as G
import echo_oracle as O
from impair_oracle import samples

pytestmark = pytest.mark.gpu

LOC_ARG = "%.6f,%.6f,%g" % LOC
CASES = O.cases_cached()
PATHS = ["carried", "plain"]


@pytest.fixture(scope="module")
def dev():
    d = G.Device(0)
    yield d
    d.close()


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    if request.param == "plain":
        monkeypatch.setenv("GSS_ECHO_PATH", "plain")
    else:
        monkeypatch.delenv("GSS_ECHO_PATH", raising=False)
    return request.param


def on_device(dev, es, blk, nch, nav, n, s0, iq, off=0):
    """gss_echo_device over iq (host int16[2 N]) placed `off` bytes into a device buffer between
    guard bytes, with the rows and tables uploaded; returns the samples"""
    import torch
    nb = 2 * len(iq)
    guard = 64
    buf = torch.full((guard + off + nb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = guard + off
    buf[lo:lo + nb] = torch.from_numpy(np.ascontiguousarray(iq).view(np.uint8)).cuda()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_blk = up(np.ascontiguousarray(blk, G.CHAN_DTYPE))
    d_nch = up(np.ascontiguousarray(nch, np.int32)) if len(nch) else torch.zeros(4, dtype=torch.uint8,
                                                                                device="cuda")
    d_ca, d_nav = up(O.ca_table()), up(np.ascontiguousarray(nav, np.uint32))
    dev.echo_device([O.to_echo(e) if isinstance(e, dict) else e for e in es], d_blk.data_ptr(),
                    d_nch.data_ptr(), len(nch), n, d_ca.data_ptr(), 32, d_nav.data_ptr(), len(nav),
                    s0, buf.data_ptr() + lo)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lo] == 0xA5).all() and (got[lo + nb:] == 0xA5).all(), "wrote outside"
    return got[lo:lo + nb].copy().view(np.int16)


@pytest.mark.parametrize("n", O.SIZES)
def test_echo_device_equals_oracle(dev, path, n):
    """the CPU test's cases of one block length: groups straddle block boundaries at every
    position, tiles hold more than two blocks below 1,023"""
    for i, c in enumerate(CASES):
        if c[5] != n:
            continue
        _, es, blk, nch, nav, _, s0, iq = c
        got = on_device(dev, es, blk, nch, nav, n, s0, iq)
        assert np.array_equal(got, O.want(i)), c[0]


def test_the_clamps(dev, path):
    for i, c in enumerate(CASES):
        if c[0].startswith("clamp"):
            _, es, blk, nch, nav, n, s0, iq = c
            assert np.array_equal(on_device(dev, es, blk, nch, nav, n, s0, iq), O.want(i)), c[0]


@pytest.mark.parametrize("off", [0, 4, 8, 12, 2, 6, 10, 14])
def test_echo_device_unaligned_base(dev, path, off):
    """the buffer at every 2-byte offset class of a 16-byte line (tests/test_gpu_impair.py's): 4,
    8 and 12 give heads of 3, 2 and 1 samples, the odd classes never line up (edges only)"""
    i = next(k for k, c in enumerate(CASES) if c[5] == 1025 and len(c[1]) == 4)
    _, es, blk, nch, nav, n, s0, iq = CASES[i]
    assert np.array_equal(on_device(dev, es, blk, nch, nav, n, s0, iq, off), O.want(i))
    i = next(k for k, c in enumerate(CASES) if c[5] == 7 and len(c[1]) == 4)
    _, es, blk, nch, nav, n, s0, iq = CASES[i]
    assert np.array_equal(on_device(dev, es, blk, nch, nav, n, s0, iq, off), O.want(i))


_stride = {}


def test_echo_device_grid_stride(dev, path):
    """one call past the grid stride (2,048 x 1,024 samples): 9 blocks of 260,000 with two pairs,
    sample0 = 2^33 + 3; the oracle once for both forms"""
    n, nblk, s0 = 260000, 9, 2 ** 33 + 3
    if not _stride:
        blk, nch, nav = O.case(n, [2] * nblk, seed=11)
        es = [O.E(O.DELAYS[2], 1 << 62, 12345 << 20, 32768, 0)]
        iq = samples(nblk * n, seed=5)
        _stride["c"] = (es, blk, nch, nav, iq, O.echo(es, blk, nch, O.ca_table(), nav, n, s0, iq))
    es, blk, nch, nav, iq, want = _stride["c"]
    assert np.array_equal(on_device(dev, es, blk, nch, nav, n, s0, iq), want)


def test_no_echo_and_empty_blocks_change_nothing(dev, path):
    i = next(k for k, c in enumerate(CASES) if c[5] == 1025 and len(c[1]) == 4)
    _, es, blk, nch, nav, n, s0, iq = CASES[i]
    assert np.array_equal(on_device(dev, [], blk, nch, nav, n, s0, iq), iq)
    assert np.array_equal(on_device(dev, es, blk, np.zeros_like(nch), nav, n, s0, iq), iq)


def test_echo_device_argument_errors(dev, path):
    """refused before any launch: the samples keep their pattern"""
    import torch
    blk, nch, nav = O.case(8, [2, 1], seed=1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_blk, d_nch, d_ca, d_nav = up(blk), up(nch), up(O.ca_table()), up(nav)
    d_iq = torch.full((64,), 0x5A5A, dtype=torch.int16, device="cuda")
    ok = G.Echo()
    good = dict(es=[ok], blk=d_blk.data_ptr(), nch=d_nch.data_ptr(), nblk=2, n=8, ca=d_ca.data_ptr(),
                n_ca=32, nav=d_nav.data_ptr(), n_nav=len(nav), s0=0, iq=d_iq.data_ptr())
    bad = [dict(es=[ok, G.Echo(delay=O.DELAY_END)]), dict(es=[ok, G.Echo(alpha_q16=(1 << 18) + 1)]),
           dict(es=[ok, G.Echo(prn=33)]), dict(es=[ok, G.Echo(prn=-1)]), dict(es=[ok] * 5),
           dict(n=0), dict(nblk=-1), dict(n_ca=0), dict(n_nav=0), dict(s0=2 ** 64 - 15),
           dict(blk=0), dict(nch=0), dict(ca=0), dict(nav=0), dict(iq=0)]
    for b in bad:
        a = dict(good, **b)
        with pytest.raises(G.GssError) as e:
            dev.echo_device(a["es"], a["blk"], a["nch"], a["nblk"], a["n"], a["ca"], a["n_ca"],
                            a["nav"], a["n_nav"], a["s0"], a["iq"])
        assert e.value.code == -1, b
    torch.cuda.synchronize()
    assert (d_iq.cpu().numpy() == 0x5A5A).all()


# ---- runs ----------------------------------------------------------------------------------------
FS = 1000000
DURATION = 0.5
IMP = {16: (256 * 300, 1), 8: (256 * 300, 3), 1: (256 * 300, 0)}      # (sigma_q8, shift)


def run_jam():
    a = G.jam_make(FS, 10.0, 137e3, 0.0, 0.0, 10e-6, 0.3)
    a.gate_shift = 7
    return [a]


def run_echoes(prn):
    """an echo of every satellite 150 m late, 6 dB down, fading at 2.5 Hz; one of satellite prn at
    40 m, 3 dB down, in anti-phase"""
    return [G.echo_make(FS, 0, 150.0, 6.0, 30.0, 2.5), G.echo_make(FS, prn, 40.0, 3.0, 180.0)]


def run_bytes(dev, fmt, impair=None, jam=None, echo=None, **kw):
    s = G.Scenario(NAV, llh=LOC, duration=DURATION, samp_freq=float(FS), data_format=fmt)
    parts, seen = [], []

    def sink(buf, first, nb):
        parts.append(bytes(buf))
        seen.append((first, nb))

    dev.run(s, sink, impair=impair, jam=jam, echo=echo, **kw)
    npb = s.n_per_blk
    s.close()
    for (a, na), (b, _) in zip(seen, seen[1:]):
        assert a + na == b
    return np.frombuffer(b"".join(parts), np.uint8), npb, seen


_run = {}


@pytest.fixture(scope="module")
def expected(dev):
    """fmt -> (gss_jam_host over gss_echo_host over the plain -b 16 run, gss_jam_host over it
    alone, n_per_blk): the plain run, the rows of a second scenario and the echoes' samples once,
    each format's bytes once"""
    def get(fmt):
        if "iq" not in _run:
            raw, npb, _ = run_bytes(dev, 16, batch=128)
            nblk = len(raw) // (4 * npb)
            assert nblk == 4
            rows = G.Scenario(NAV, llh=LOC, duration=DURATION, samp_freq=float(FS))
            blk, nch = rows.all_blocks()
            nav = rows.nav_table()
            rows.close()
            assert len(nch) == nblk
            prn = int(blk[0, 0]["ca_tbl"]) + 1
            iq = raw.view(np.int16)
            mid = G.echo_host(run_echoes(prn), blk, nch, G.ca_table(), nav, npb, 0, iq)
            assert not np.array_equal(mid, iq)
            _run["iq"] = (iq, mid, npb, prn)
        iq, mid, npb, prn = _run["iq"]
        if fmt not in _run:
            imp = G.Impair(*IMP[fmt], 7)
            _run[fmt] = (G.jam_host(imp, run_jam(), mid, 0, fmt), G.jam_host(imp, run_jam(), iq, 0, fmt))
        return _run[fmt] + (npb, prn)
    return get


MODES = {
    "batch2": ({}, dict(batch=2)),
    "batch128": ({}, dict(batch=128)),
    "range": ({}, dict(batch=3, first_block=1, n_blocks=2)),
    "gpu_exact3_late": ({"GSS_RUN_PROOF": "gpu", "GSS_RUN_FORCE_EXACT": "3",
                         "GSS_RUN_LATE_VERDICTS": "1"}, dict(batch=4)),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_run_with_noise_a_jammer_and_echoes(dev, expected, monkeypatch, fmt, mode):
    want, _, npb, prn = expected(fmt)               # (the plain run before the mode's environment)
    env, kw = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, _, seen = run_bytes(dev, fmt, impair=G.Impair(*IMP[fmt], 7), jam=run_jam(),
                             echo=run_echoes(prn), threads=4, **kw)
    if mode == "range":
        bb = G.block_bytes(npb, fmt)
        assert seen[0][0] == 1 and sum(nb for _, nb in seen) == 2
        assert np.array_equal(got, want[bb:3 * bb])
    else:
        assert sum(nb for _, nb in seen) == 4
        assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", [16, 8, 1])
def test_run_without_echoes_is_the_parents(dev, expected, fmt):
    """echo=None and echo=[]: the jammer's bytes; echoes without an impairment: refused"""
    _, want, _, prn = expected(fmt)
    for echo in (None, []):
        got, _, _ = run_bytes(dev, fmt, impair=G.Impair(*IMP[fmt], 7), jam=run_jam(), echo=echo,
                              batch=4)
        assert np.array_equal(got, want)
    with pytest.raises(G.GssError) as e:
        run_bytes(dev, fmt, impair=None, echo=run_echoes(prn), batch=4)
    assert e.value.code == -1


def test_cli_multipath(dev, expected, tmp_path):
    """gps-sdr-sim --multipath=... writes the host composition over the plain run, with the echoes
    the parser resolves, and one stderr line per echo"""
    _, _, npb, prn = expected(8)
    iq, _, _, _ = _run["iq"]
    opts = ["--cn0=45", "--seed=7", "--jam=cw,10,137e3,pulse,10e-6,0.3", "--multipath=all,150,6,30,2.5",
            "--multipath=%d,40,3,180" % prn]
    args = ["-e", NAV, "-l", LOC_ARG, "-d", str(DURATION), "-s", str(FS), "-b", "8"]
    out = tmp_path / "echoed.bin"
    p = subprocess.run([G.CLI_PATH] + args + ["-o", str(out)] + opts, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr.count("\nEcho ") == 2 and "Noise: " in p.stderr
    scn, _ = G.Scenario.from_cli(args + opts)
    imp, js, es = scn.impair, scn.jam, scn.echo
    blk, nch = scn.all_blocks()
    nav = scn.nav_table()
    scn.close()
    assert len(es) == 2 and es[0].prn == 0 and es[1].prn == prn
    mid = G.echo_host(es, blk, nch, G.ca_table(), nav, npb, 0, iq)
    assert np.array_equal(np.fromfile(out, np.uint8), G.jam_host(imp, js, mid, 0, 8))
