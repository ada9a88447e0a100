"""The host's run-ahead carrier walk (gss_spec_host: gss_spec_guess_row and gss_spec_seg_walk,
gss_phase.h) on the synthetic rows of tests/spec_oracle.py against brute force: steps from a few
Hz at 2.6 MS/s to 0.45 cycles per sample, powers of two, rounding ties, 1/s next to an integer,
starts 0 and 1 - 2^-53, and blocks from one sample to two million.  Every walked segment's
interval of exact start translations is checked at both of its ends (check_walks).  The GPU walks
are compared with these (tests/test_gpu_spec_walk.py), so this is the soundness of that
reference on the whole domain."""
import numpy as np
import pytest

import gpssim_amd as G
import spec_oracle as O

NS = [1, 33, 4100, 100000, 260000, 2000000]


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", NS)
def test_host_walks_synthetic(n, seed):
    gi = O.spec_in(O.rows(seed, 160))
    spec = G.spec_host(gi, n, threads=4)
    assert np.all(gi["k"] >= 1) and np.all(gi["pad"] == -1)
    checks = O.check_walks(gi, spec, n)
    if n >= 4100:                       # no guesses (fewer than two wraps) and all of them
        assert np.any(gi["k"] == 1) and np.any(gi["k"] == G.SPEC_K), np.bincount(gi["k"])
        assert checks > 0
    print(f"n={n} seed={seed}: {checks} translation checks, k histogram {np.bincount(gi['k'])}")


@pytest.mark.parametrize("n", [33, 4100, 260000])
def test_power_of_two_steps_from_lattice_starts(n):
    """LATTICE_ROWS: exact ends and wraps, and every interval reported holds 0 and is sound"""
    gi = O.spec_in(O.LATTICE_ROWS)
    assert np.all(O.on_lattice(gi))
    spec = G.spec_host(gi, n, threads=1)
    O.check_walks(gi, spec, n)
    seg = spec["seg"]
    kept = seg["dlo"] <= seg["dhi"]
    assert np.all((seg["dlo"][kept] <= 0) & (seg["dhi"][kept] >= 0))
    assert np.all((seg["dlo"][~kept] == 1.0) & (seg["dhi"][~kept] == 0.0))


def test_rows_are_deterministic_and_cover_the_families():
    a, b = O.rows(5, 400), O.rows(5, 400)
    assert a == b and a != O.rows(6, 400)
    g = np.array([r[0] for r in a])
    s = np.array([r[1] for r in a])
    assert np.all(s != 0) and np.all(np.abs(s) <= 0.45 + 2.0 ** -53)
    assert np.any(g == 0.0) and np.any(g == O.TOP)
    assert np.any(s > 0.4) and np.any(s < -0.4)
    assert np.any(np.abs(s) * 260000 < 1)                          # no wrap in a 0.1 s block
    m = np.abs(s) * 2.0 ** 53
    assert np.sum(m - np.floor(m) == 0.5) >= 400 // 7               # the ties
    e = np.log2(np.abs(s))
    assert np.sum(e == np.round(e)) >= 400 // 7 - 400 // 49 - 1     # the powers of two
