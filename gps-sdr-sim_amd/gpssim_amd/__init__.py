"""Python binding of libgpssim_amd.so (C ABI declared in include/gpssim_amd.h).

The product is the C library: a host control plane (gss_scn_*) mirroring gpssim.c's main() and a
gfx950 HIP hot path (gss_synth_*) replacing its per-sample loop (gpssim.c:2190-2288).  This module
is plumbing for the tests and bench: ctypes prototypes, numpy views of the parameter rows, and
thin wrappers.  There is no Python or CPU implementation of the synthesis here: when the shared
library or a GPU is missing, the calls raise.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_DIR = os.path.dirname(PKG_DIR)
# The in-tree build (make -C gps-sdr-sim_amd).  Measurement builds of kernel variants
# (tools/ablate.sh) load only with both GSS_LIB_PATH and GSS_ALLOW_LIB_OVERRIDE=1 set; bench.py
# records the path it measured and the tests refuse to run on anything but the in-tree build.
_INTREE = os.path.join(PKG_DIR, "lib", "libgpssim_amd.so")
if os.environ.get("GSS_LIB_PATH") and os.environ.get("GSS_ALLOW_LIB_OVERRIDE") != "1":
    raise ImportError("GSS_LIB_PATH is set without GSS_ALLOW_LIB_OVERRIDE=1: refusing to load a "
                      "library other than the in-tree build " + _INTREE)
LIB_PATH = os.environ.get("GSS_LIB_PATH") or _INTREE
IN_TREE = os.path.abspath(LIB_PATH) == os.path.abspath(_INTREE)
CLI_PATH = os.path.join(PKG_DIR, "bin", "gps-sdr-sim")
ACQ_CLI_PATH = os.path.join(PKG_DIR, "bin", "gps-sdr-acq")
TRK_CLI_PATH = os.path.join(PKG_DIR, "bin", "gps-sdr-track")
PVT_CLI_PATH = os.path.join(PKG_DIR, "bin", "gps-sdr-pvt")

MAXCH = 16
CA_WORDS = 32
NAV_WORDS = 60
NCK = 8                       # GSS_NCK: carrier checkpoints per block (gss_scn_next)
FMT_SC01, FMT_SC08, FMT_SC16 = 1, 8, 16

# gss_chan_blk_t (56 bytes), gpssim_amd.h
CHAN_DTYPE = np.dtype([
    ("carr0", "<f8"), ("carr_step", "<f8"), ("code0", "<f8"), ("code_step", "<f8"),
    ("icode", "<i4"), ("ibit", "<i4"), ("iword", "<i4"), ("gain", "<i4"),
    ("ca_tbl", "<i4"), ("nav_tbl", "<i4"),
])
assert CHAN_DTYPE.itemsize == 56

NGC = 8                       # GSS_NGC: signed-gain schedule entries
NPATCH = 8                    # GSS_NPATCH: patched samples per block and channel
# gss_lin_t (192 bytes): certified integer lines of one block and channel, gpssim_amd.h
LIN_DTYPE = np.dtype([
    ("x0", "<u8"), ("xs", "<u8"), ("z0", "<u8"), ("zs", "<u8"),
    ("pdelta", "<i8", (NPATCH,)),
    ("gpos", "<i4", (NGC,)), ("gval", "<i4", (NGC,)), ("ppos", "<i4", (NPATCH,)),
])
assert LIN_DTYPE.itemsize == 192

# gss_chain_t (16 bytes): the carrier chain a (block, channel) row continues, gpssim_amd.h
CHAIN_DTYPE = np.dtype([("slot", "i1"), ("reset", "u1"), ("pad", "u1", (6,)), ("init", "<f8")])
assert CHAIN_DTYPE.itemsize == 16
# the carrier chain run ahead (gss_carr_chain_guess / gss_spec_* / gss_carr_chain_spec)
# speculative segments per block (GSS_SPEC_K: 32 in the product build; a measurement build of
# another value is loaded with GSS_SPEC_K set to it as well -- lib() checks that the library
# agrees, without loading it at import: torch must load its HIP runtime first)
SPEC_K = int(os.environ.get("GSS_SPEC_K", "32"))
SPEC_IN_DTYPE = np.dtype([("g", "<f8"), ("s", "<f8"), ("k", "<i4"), ("pad", "<i4"),
                          ("P", "<i8", (SPEC_K,)), ("W", "<f8", (SPEC_K,))])
assert SPEC_IN_DTYPE.itemsize == 24 + 16 * SPEC_K
SPEC_SEG_DTYPE = np.dtype([("end", "<f8"), ("dlo", "<f8"), ("dhi", "<f8"), ("wrap_end", "<i8")])
SPEC_DTYPE = np.dtype([("p1", "<i8"), ("w1", "<f8"), ("seg", SPEC_SEG_DTYPE, (SPEC_K,))])
assert SPEC_DTYPE.itemsize == 16 + 32 * SPEC_K
SPEC_LINK_DTYPE = np.dtype([("lo", "<f8"), ("hi", "<f8"), ("dd", "<f8"), ("end", "<f8")])
assert SPEC_LINK_DTYPE.itemsize == 32
# gss_spec_rec_t: a row's speculative walk folded into one record (gss_spec_records*)
SPEC_REC_DTYPE = np.dtype([("w1", "<f8"), ("slo", "<f8"), ("shi", "<f8"), ("sdd", "<f8"),
                           ("end", "<f8"), ("llo", "<f8"), ("lhi", "<f8"), ("ldd", "<f8"),
                           ("p1", "<i4"), ("ok", "<i4")])
assert SPEC_REC_DTYPE.itemsize == 72
# gss_carr_anchor_t: the chain's exact carrier values inside a block (the proofs' walk starts)
ANCHOR_DTYPE = np.dtype([("pos", "<i4", (SPEC_K,)), ("val", "<f8", (SPEC_K,))])
assert ANCHOR_DTYPE.itemsize == 12 * SPEC_K
# gss_nav_src_t: one nav-table row's source for the GPU producer (include/gpssim_amd.h)
NAV_SRC_DTYPE = np.dtype([("sbf", "<u4", (5, 10)), ("tow", "<u4"), ("wn", "<u4"), ("prev", "<i4"),
                          ("next", "<i4"), ("head", "<u4", (10,))])
assert NAV_SRC_DTYPE.itemsize == 256
NAV_HEAD_INIT, NAV_HEAD_GIVEN = -1, -2
# gss_acq_peak_t: one PRN's peak and floor of the acquisition search (gss_acquire_*)
ACQ_PEAK_DTYPE = np.dtype([("peak", "<u8"), ("floor_sum", "<u8"), ("floor_cnt", "<u4"),
                           ("tau", "<i4"), ("bin", "<i4"), ("prn", "<i4")])
assert ACQ_PEAK_DTYPE.itemsize == 32
# gss_trk_rec_t: one code period of one tracking job (gss_track_*)
TRK_REC_DTYPE = np.dtype([("IE", "<i8"), ("QE", "<i8"), ("IP", "<i8"), ("QP", "<i8"),
                          ("IL", "<i8"), ("QL", "<i8"), ("s", "<i8"), ("w", "<i4"),
                          ("dcs", "<i4")])
assert TRK_REC_DTYPE.itemsize == 64
# gss_trk_job_t: where a tracking job starts (gss_trk_job_from_peak)
TRK_JOB_DTYPE = np.dtype([("s0", "<i8"), ("prn", "<i4"), ("w0", "<i4"), ("n_epoch", "<i4"),
                          ("pad", "<i4")])
assert TRK_JOB_DTYPE.itemsize == 24
# gss_nav_sf_t: one decoded subframe (gss_nav_decode)
NAV_SF_DTYPE = np.dtype([("sample", "<i8"), ("epoch", "<i4"), ("polarity", "<i4"),
                         ("tow", "<i4"), ("id", "<i4"), ("word", "<u4", (10,))])
assert NAV_SF_DTYPE.itemsize == 64
# gss_obs_t: code phase and accumulated carrier of one job at one instant (gss_obs_*)
OBS_DTYPE = np.dtype([("code", "<i8"), ("adr", "<i8"), ("epoch", "<i4"), ("w", "<i4"),
                      ("pad", "<i8")])
assert OBS_DTYPE.itemsize == 32
# gss_pvt_sat_t: one satellite of a fix (gss_pvt_solve)
PVT_SAT_DTYPE = np.dtype([("obs", OBS_DTYPE), ("prn", "<i4"), ("sf_epoch", "<i4"),
                          ("sf_tow", "<i4"), ("pad", "<i4")])
assert PVT_SAT_DTYPE.itemsize == 48
NAVDATA_FIELDS = ("valid", "iode", "iodc", "toc", "toe", "af0", "af1", "af2", "tgd", "crs",
                  "deltan", "m0", "cuc", "ecc", "cus", "sqrta", "cic", "omg0", "cis", "inc0",
                  "crc", "aop", "omgdot", "idot", "iono_valid", "alpha0", "alpha1", "alpha2",
                  "alpha3", "beta0", "beta1", "beta2", "beta3", "week")   # GSS_NAVDATA_FIELDS
PVT_OK, PVT_FEW, PVT_SINGULAR, PVT_DIVERGED = 0, 1, 2, 3


class GssError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gpssim_amd error {code}: {msg}")
        self.code = code


class _Opts(C.Structure):
    _fields_ = [
        ("nav_file", C.c_char_p), ("motion_file", C.c_char_p), ("nmea", C.c_int),
        ("has_xyz", C.c_int), ("xyz", C.c_double * 3), ("has_llh", C.c_int),
        ("llh", C.c_double * 3), ("samp_freq", C.c_double), ("data_format", C.c_int),
        ("duration", C.c_double), ("has_start", C.c_int), ("time_overwrite", C.c_int),
        ("start", C.c_int * 6), ("start_sec", C.c_double), ("iono_disable", C.c_int),
        ("verbose", C.c_int), ("user_motion_size", C.c_int), ("quiet", C.c_int),
        ("carrier_int", C.c_int),
    ]


class Impair(C.Structure):
    """gss_impair_t: seeded additive Gaussian noise, sigma_q8 / 256 LSB of the 16-bit sample per
    component, after which every sample is shifted right by `shift` (0..8) with rounding."""
    _fields_ = [("seed", C.c_uint64), ("sigma_q8", C.c_uint32), ("shift", C.c_int32)]

    def __init__(self, sigma_q8=0, shift=0, seed=0):
        super().__init__(int(seed), int(sigma_q8), int(shift))

    def __repr__(self):
        return f"Impair(sigma_q8={self.sigma_q8}, shift={self.shift}, seed={self.seed})"


MAXJAM = 4                                         # GSS_MAXJAM


class Jam(C.Structure):
    """gss_jam_t: one jammer in the definition's integers (include/gpssim_amd.h); jam_make() fills
    one from physical parameters."""
    _fields_ = [("step0", C.c_uint64), ("rate", C.c_uint64), ("phase0", C.c_uint64),
                ("sweep", C.c_uint32), ("amp", C.c_uint32), ("gate_period", C.c_uint32),
                ("gate_on", C.c_uint32), ("gate_shift", C.c_uint32), ("pad", C.c_uint32)]

    def __init__(self, step0=0, rate=0, phase0=0, sweep=1, amp=0, gate_period=0, gate_on=0,
                 gate_shift=0, pad=0):
        m = 2**64 - 1
        super().__init__(int(step0) & m, int(rate) & m, int(phase0) & m, int(sweep), int(amp),
                         int(gate_period), int(gate_on), int(gate_shift), int(pad))

    def __repr__(self):
        return (f"Jam(step0={self.step0}, rate={self.rate}, phase0={self.phase0}, "
                f"sweep={self.sweep}, amp={self.amp}, gate_period={self.gate_period}, "
                f"gate_on={self.gate_on}, gate_shift={self.gate_shift}, pad={self.pad})")


MAXECHO = 4                                        # GSS_MAXECHO


class Echo(C.Structure):
    """gss_echo_t: one multipath echo in the definition's integers (include/gpssim_amd.h);
    echo_make() fills one from physical parameters."""
    _fields_ = [("delay", C.c_uint64), ("theta0", C.c_uint64), ("dstep", C.c_uint64),
                ("alpha_q16", C.c_uint32), ("prn", C.c_int32)]

    def __init__(self, delay=0, theta0=0, dstep=0, alpha_q16=65536, prn=0):
        m = 2**64 - 1
        super().__init__(int(delay) & m, int(theta0) & m, int(dstep) & m, int(alpha_q16), int(prn))

    def __repr__(self):
        return (f"Echo(delay={self.delay}, theta0={self.theta0}, dstep={self.dstep}, "
                f"alpha_q16={self.alpha_q16}, prn={self.prn})")


MAXTAP = 64                                        # GSS_MAXTAP


class Fir(C.Structure):
    """gss_fir_t: the front-end filter's Q14 taps (include/gpssim_amd.h); fir_make() designs a
    low-pass, Fir(taps=[...]) takes any taps."""
    _fields_ = [("n_taps", C.c_int32), ("pad", C.c_int32), ("taps", C.c_int16 * MAXTAP)]

    def __init__(self, taps=(), n_taps=None, pad=0):
        taps = [int(t) for t in taps]
        if len(taps) > MAXTAP:
            raise ValueError(f"Fir: at most {MAXTAP} taps")
        super().__init__(len(taps) if n_taps is None else int(n_taps), int(pad),
                         (C.c_int16 * MAXTAP)(*taps))

    def tap_list(self):
        return [int(self.taps[k]) for k in range(max(0, min(self.n_taps, MAXTAP)))]

    def __repr__(self):
        return f"Fir(n_taps={self.n_taps}, pad={self.pad}, taps={self.tap_list()})"


class Acq(C.Structure):
    """gss_acq_t: an acquisition search.  fs_hz, fmt (16 / 8 / 1), coh_ms x n_coh windows, bins
    -n_half..n_half of bin_hz (default 500 / coh_ms), qshift (-1: auto), prns (iterable of 1..32,
    default all)."""
    _fields_ = [("fs_hz", C.c_int32), ("fmt", C.c_int32), ("coh_ms", C.c_int32),
                ("n_coh", C.c_int32), ("bin_hz", C.c_int32), ("n_half", C.c_int32),
                ("qshift", C.c_int32), ("prn_mask", C.c_uint32)]

    def __init__(self, fs_hz, fmt=16, coh_ms=1, n_coh=10, bin_hz=None, n_half=20, qshift=-1,
                 prns=None):
        mask = 0xFFFFFFFF
        if prns is not None:
            mask = 0
            for p in prns:
                if not 1 <= int(p) <= 32:
                    raise ValueError(f"PRN {p} outside 1..32")
                mask |= 1 << (int(p) - 1)
        super().__init__(int(fs_hz), int(fmt), int(coh_ms), int(n_coh),
                         int(500 // max(int(coh_ms), 1) if bin_hz is None else bin_hz),
                         int(n_half), int(qshift), mask)

    def sizes(self):
        """(L, T, N, E, n_prn): samples per window, code phases, samples read, excluded
        half-width, selected PRNs (gss_acq_sizes)"""
        L, T, E, P = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        N = C.c_int64()
        _check(lib().gss_acq_sizes(C.byref(self), C.byref(L), C.byref(T), C.byref(N),
                                   C.byref(E), C.byref(P)))
        return L.value, T.value, N.value, E.value, P.value

    def sample_bytes(self):
        """bytes the search reads from its sample pointer"""
        n = self.sizes()[2]
        return {FMT_SC16: 4 * n, FMT_SC08: 2 * n, FMT_SC01: (n + 3) // 4}[self.fmt]


class Trk(C.Structure):
    """gss_trk_cfg_t: the tracking loops.  Trk(fs_hz, fmt) holds the default gains
    (gss_trk_defaults); keyword arguments n_pull, Kf, Ki, Kp, Kd replace single fields."""
    _fields_ = [("fs_hz", C.c_int32), ("fmt", C.c_int32), ("n_pull", C.c_int32),
                ("Kf", C.c_int32), ("Ki", C.c_int32), ("Kp", C.c_int32), ("Kd", C.c_int32)]

    def __init__(self, fs_hz, fmt=16, **over):
        super().__init__()
        _check(lib().gss_trk_defaults(int(fs_hz), int(fmt), C.byref(self)))
        for k, v in over.items():
            if k not in ("n_pull", "Kf", "Ki", "Kp", "Kd"):
                raise TypeError(f"unknown field {k}")
            setattr(self, k, int(v))

    def __repr__(self):
        return (f"Trk(fs_hz={self.fs_hz}, fmt={self.fmt}, n_pull={self.n_pull}, Kf={self.Kf}, "
                f"Ki={self.Ki}, Kp={self.Kp}, Kd={self.Kd})")


class _PvtOpts(C.Structure):                         # gss_pvt_opts_t
    _fields_ = [("no_iono", C.c_int32), ("week", C.c_int32)]


class PvtFix(C.Structure):
    """gss_pvt_fix_t: what gss_pvt_solve returns (status PVT_OK, PVT_FEW, PVT_SINGULAR or
    PVT_DIVERGED; T0 = t0_floor + t0_frac seconds of week t0_week)"""
    _fields_ = [("xyz", C.c_double * 3), ("llh", C.c_double * 3), ("vel", C.c_double * 3),
                ("t0_sec", C.c_double), ("t0_frac", C.c_double), ("t0_floor", C.c_double),
                ("drift", C.c_double), ("pdop", C.c_double), ("rms", C.c_double),
                ("t0_week", C.c_int32), ("n_used", C.c_int32), ("status", C.c_int32),
                ("iterations", C.c_int32)]


class _Truth(C.Structure):                           # gss_acq_truth_t
    _fields_ = [("tau", C.c_double), ("doppler_hz", C.c_double), ("cn0_offset_db", C.c_double),
                ("prn", C.c_int32), ("pad", C.c_int32)]


class _Cli(C.Structure):
    _fields_ = [("opt", _Opts), ("nav_file", C.c_char * 256), ("motion_file", C.c_char * 256),
                ("out_file", C.c_char * 256), ("impair", Impair), ("has_impair", C.c_int),
                ("jam", Jam * MAXJAM), ("n_jam", C.c_int),
                ("echo", Echo * MAXECHO), ("n_echo", C.c_int),
                ("fir", Fir), ("has_fir", C.c_int)]


class _RunOpts(C.Structure):                         # gss_run_opts_t
    _fields_ = [("carr_in", C.c_void_p), ("carr_out", C.c_void_p), ("carr_user", C.c_void_p),
                ("carr_predict", C.c_void_p), ("impair", C.POINTER(Impair)),
                ("jam", C.POINTER(Jam)), ("n_jam", C.c_int),
                ("echo", C.POINTER(Echo)), ("n_echo", C.c_int),
                ("fir", C.POINTER(Fir))]


class _Info(C.Structure):
    _fields_ = [("n_per_blk", C.c_int), ("n_blocks", C.c_int), ("data_format", C.c_int),
                ("samp_freq", C.c_double), ("delt", C.c_double), ("week", C.c_int),
                ("sec", C.c_double), ("next_block", C.c_int64), ("rows_out", C.c_int64),
                ("carrier_int", C.c_int)]


_lib = None

# name -> (restype, argtypes); every symbol include/gpssim_amd.h declares
_P = C.c_void_p
# gss_sink_fn(user, bytes, n, first_block, nblocks)
SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int)
_SIGS = {
    "gss_run": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, C.c_int, SINK_FN, _P]),
    "gss_run_ex": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, C.c_int, SINK_FN, _P, _P]),
    "gss_dev_open": (C.c_int, [C.POINTER(_P), C.c_int]),
    "gss_dev_close": (C.c_int, [_P]),
    "gss_dev_reserve": (C.c_int, [_P, C.c_int, C.c_int]),
    "gss_block_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "gss_anchor_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P,
                                    _P]),
    "gss_render_device": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, C.c_int,
                                    C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "gss_synth_device": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, C.c_int, _P, C.c_int,
                                   C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "gss_synth_host": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                 C.c_int, _P, _P]),
    "gss_linearize": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P,
                                C.c_int]),
    "gss_linearize_device": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P,
                                       _P, _P]),
    "gss_synth_lin_device": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P,
                                       C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                       _P]),
    "gss_minmax_mod": (None, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gss_first_below": (C.c_uint64, [C.c_uint64] * 5),
    "gss_hits_mod": (C.c_int, [C.c_uint64] * 5 + [_P, C.c_int, C.c_int]),
    "gss_noise_table": (C.c_int, [_P]),
    "gss_impair_host": (C.c_int, [C.POINTER(Impair), _P, C.c_uint64, C.c_size_t, C.c_int, _P]),
    "gss_impair_device": (C.c_int, [_P, C.POINTER(Impair), _P, C.c_uint64, C.c_size_t, C.c_int,
                                    _P, _P]),
    "gss_jam_make": (C.c_int, [C.c_double] * 7 + [C.POINTER(Jam)]),
    "gss_jam_host": (C.c_int, [C.POINTER(Impair), C.POINTER(Jam), C.c_int, _P, C.c_uint64,
                               C.c_size_t, C.c_int, _P]),
    "gss_jam_device": (C.c_int, [_P, C.POINTER(Impair), C.POINTER(Jam), C.c_int, _P, C.c_uint64,
                                 C.c_size_t, C.c_int, _P, _P]),
    "gss_echo_make": (C.c_int, [C.c_double, C.c_int] + [C.c_double] * 4 + [C.POINTER(Echo)]),
    "gss_echo_check": (C.c_int, [C.POINTER(Echo), C.c_int]),
    "gss_echo_host": (C.c_int, [C.POINTER(Echo), C.c_int, _P, _P, C.c_int, C.c_int, _P, C.c_int,
                                _P, C.c_int, C.c_uint64, _P]),
    "gss_echo_device": (C.c_int, [_P, C.POINTER(Echo), C.c_int, _P, _P, C.c_int, C.c_int, _P,
                                  C.c_int, _P, C.c_int, C.c_uint64, _P, _P]),
    "gss_fir_make": (C.c_int, [C.c_double, C.c_double, C.c_int, C.POINTER(Fir)]),
    "gss_fir_check": (C.c_int, [C.POINTER(Fir)]),
    "gss_fir_host": (C.c_int, [C.POINTER(Fir), _P, _P, C.c_size_t, C.c_int, _P]),
    "gss_fir_device": (C.c_int, [_P, C.POINTER(Fir), _P, _P, C.c_size_t, C.c_int, _P, _P]),
    "gss_acq_sizes": (C.c_int, [C.POINTER(Acq), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32)]),
    "gss_acquire_host": (C.c_int, [C.POINTER(Acq), _P, _P, _P, C.POINTER(C.c_int), C.c_int]),
    "gss_acquire_device": (C.c_int, [_P, C.POINTER(Acq), _P, _P, _P, _P, _P]),
    "gss_acquire": (C.c_int, [_P, C.POINTER(Acq), _P, _P, _P, C.POINTER(C.c_int)]),
    "gss_acq_expect": (C.c_int, [_P, C.c_double, C.c_int64, C.POINTER(_Truth)]),
    "gss_acq_threshold": (C.c_double, [C.c_int, C.c_uint64, C.c_double]),
    "gss_trk_defaults": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Trk)]),
    "gss_trk_job_from_peak": (C.c_int, [C.POINTER(Acq), _P, C.c_int64, C.c_int32, _P]),
    "gss_track_host": (C.c_int, [C.POINTER(Trk), _P, C.c_int64, _P, C.c_int, _P, C.c_int64, _P,
                                 C.c_int]),
    "gss_track_device": (C.c_int, [_P, C.POINTER(Trk), _P, C.c_int64, _P, C.c_int, _P, C.c_int64,
                                   _P, _P]),
    "gss_track": (C.c_int, [_P, C.POINTER(Trk), _P, C.c_int64, _P, C.c_int, _P, C.c_int64, _P]),
    "gss_nav_decode": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int, C.POINTER(C.c_int32)]),
    "gss_trk_cn0": (C.c_double, [_P, C.c_int64, C.c_int64]),
    "gss_obs_host": (C.c_int, [C.c_int32, _P, C.c_int64, _P, C.c_int, C.c_int64, C.c_int64,
                               C.c_int32, _P, C.c_int]),
    "gss_obs_device": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, C.c_int, C.c_int64, C.c_int64,
                                 C.c_int32, _P, _P]),
    "gss_obs": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, C.c_int, C.c_int64, C.c_int64,
                          C.c_int32, _P]),
    "gss_navdata_open_rinex": (C.c_int, [C.POINTER(_P), C.c_char_p]),
    "gss_navdata_open_empty": (C.c_int, [C.POINTER(_P)]),
    "gss_navdata_add_subframe": (C.c_int, [_P, C.c_int, _P]),
    "gss_navdata_get": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "gss_navdata_close": (C.c_int, [_P]),
    "gss_pvt_solve": (C.c_int, [_P, C.c_double, C.c_int64, _P, C.c_int, C.POINTER(_PvtOpts),
                                C.POINTER(PvtFix)]),
    "gss_pvt_range": (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.c_int, _P]),
    "gss_dev_timing": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float),
                                 C.POINTER(C.c_float)]),
    "gss_dev_timing_lin": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "gss_scn_open": (C.c_int, [C.POINTER(_P), C.POINTER(_Opts)]),
    "gss_scn_info": (C.c_int, [_P, C.POINTER(_Info)]),
    "gss_scn_next": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_int), C.c_int]),
    "gss_scn_next_deferred": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_int), C.c_int]),
    "gss_carr_chain": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "gss_carr_chain_guess": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "gss_carr_chain_starts": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "gss_carr_line_end": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "gss_spec_host": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int]),
    "gss_spec_device": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "gss_carr_chain_spec": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int,
                                      C.POINTER(C.c_int)]),
    "gss_spec_links": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int]),
    "gss_carr_chain_anchored": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int,
                                          C.POINTER(C.c_int), _P]),
    "gss_carr_anchors": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int]),
    "gss_spec_records": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "gss_spec_records_device": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "gss_carr_chain_records": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int,
                                         C.POINTER(C.c_int)]),
    "gss_linearize_ex": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, _P,
                                   C.c_int]),
    "gss_linearize_device_ex": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int,
                                          _P, _P, _P, _P]),
    "gss_carr_chain_linked": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int,
                                        C.POINTER(C.c_int)]),
    "gss_scn_seek": (C.c_int, [_P, C.c_int64, C.c_int]),
    "gss_scn_carrier": (C.c_int, [_P, _P]),
    "gss_scn_set_carrier": (C.c_int, [_P, _P]),
    "gss_scn_nav_table": (C.c_int, [_P, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_int)]),
    "gss_ca_table": (C.c_int, [_P]),
    "gss_scn_nav_sources": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int)]),
    "gss_nav_rows_host": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "gss_nav_rows_device": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "gss_ca_table_device": (C.c_int, [_P, _P, _P]),
    "gss_scn_plan_seconds": (C.c_double, [_P]),
    "gss_scn_close": (C.c_int, [_P]),
    "gss_carr_advance": (C.c_double, [C.c_double, C.c_double, C.c_int64]),
    "gss_carr_advance_ck": (C.c_double, [C.c_double, C.c_double, C.c_int, C.c_void_p]),
    "gss_code_advance": (C.c_double, [C.c_double, C.c_double, C.c_int64,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]),
    "gss_lut": (C.c_int, [_P, _P]),
    "gss_cli_parse": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(_Cli)]),
    "gss_cli_usage": (None, []),
    "gss_last_error": (C.c_char_p, []),
    "gss_version": (C.c_char_p, []),
    "gss_build_info": (C.c_char_p, []),
}
EXPORTED = tuple(_SIGS)


def lib():
    """Load the in-tree shared library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} missing: run `make -C gps-sdr-sim_amd` "
                          "(or __graft_entry__.build())")
        try:
            # A process that also uses PyTorch-ROCm must resolve libamdhip64 to torch's copy:
            # load torch first so the library binds to the already-loaded runtime (two HIP
            # runtimes in one process leave torch seeing no GPU).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        kv = dict(x.split("=", 1) for x in L.gss_build_info().decode().split())
        if int(kv.get("spec_k", "8")) != SPEC_K:          # (builds before round 6: 8)
            raise ImportError(f"{LIB_PATH} was built with GSS_SPEC_K={kv.get('spec_k')}: set "
                              f"GSS_SPEC_K to match (Python's walk dtypes use {SPEC_K})")
        _lib = L
    return _lib


def build_info():
    """The kernels' build configuration as a dict, e.g. {"lin_mfma": "1", "lin_ch": "16", ...}."""
    return dict(kv.split("=", 1) for kv in lib().gss_build_info().decode().split())


def lib_mfma():
    """True when the fast path accumulates on the matrix cores (LIN_MFMA build)."""
    return build_info().get("lin_mfma", "0") != "0"


def _check(rc):
    if rc != 0:
        raise GssError(rc, lib().gss_last_error().decode(errors="replace"))


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def block_bytes(n_per_blk, fmt):
    return int(lib().gss_block_bytes(n_per_blk, fmt))


def ca_table():
    out = np.zeros((32, CA_WORDS), np.uint32)
    _check(lib().gss_ca_table(_ptr(out)))
    return out


def nav_rows_host(src, first=0, rows=None):
    """rows [first, first + len(src)) from their sources (gss_nav_rows_host); rows: the table so
    far (>= first rows), extended and returned"""
    src = np.ascontiguousarray(src, NAV_SRC_DTYPE)
    out = np.zeros((first + len(src), NAV_WORDS), np.uint32)
    if first:
        out[:first] = rows[:first]
    _check(lib().gss_nav_rows_host(_ptr(src), first, len(src), _ptr(out)))
    return out


def noise_table():
    """the half-normal inverse-CDF table of the additive noise (gss_noise_table): int32[4097]"""
    out = np.zeros(4097, np.int32)
    _check(lib().gss_noise_table(_ptr(out)))
    return out


def impair_bytes(n, fmt):
    """bytes n impaired samples take in format fmt"""
    return {FMT_SC16: 4 * n, FMT_SC08: 2 * n, FMT_SC01: n // 4}[fmt]


def impair_host(imp, iq, sample0, fmt):
    """The impairment on the host (gss_impair_host): iq int16[2 n], the noise-free components of
    samples [sample0, sample0 + n); returns the bytes of format fmt as uint8."""
    iq = np.ascontiguousarray(iq, np.int16).reshape(-1)
    n = len(iq) // 2
    out = np.zeros(impair_bytes(n, fmt) if fmt in (1, 8, 16) else 0, np.uint8)
    _check(lib().gss_impair_host(C.byref(imp), _ptr(iq), int(sample0), n, int(fmt), _ptr(out)))
    return out


def _jam_array(jam):
    """(ctypes array or None, count) of an iterable of Jam; the count is passed on as it is, so
    that the library refuses more than MAXJAM"""
    jam = list(jam or ())
    return ((Jam * len(jam))(*jam) if jam else None), len(jam)


def jam_make(fs_hz, js_db, f0_hz, f1_hz=0.0, sweep_s=0.0, gate_period_s=0.0, duty=0.0):
    """A Jam from physical parameters (gss_jam_make): J/S in dB against a satellite at gain 128,
    a tone at f0_hz (sweep_s 0) or a sweep f0_hz -> f1_hz every sweep_s seconds, optionally pulsed
    with gate_period_s and duty."""
    j = Jam()
    _check(lib().gss_jam_make(float(fs_hz), float(js_db), float(f0_hz), float(f1_hz),
                              float(sweep_s), float(gate_period_s), float(duty), C.byref(j)))
    return j


def jam_host(imp, jam, iq, sample0, fmt):
    """gss_jam_host: impair_host with the jammers `jam` (an iterable of Jam) added."""
    iq = np.ascontiguousarray(iq, np.int16).reshape(-1)
    n = len(iq) // 2
    out = np.zeros(impair_bytes(n, fmt) if fmt in (1, 8, 16) else 0, np.uint8)
    arr, nj = _jam_array(jam)
    _check(lib().gss_jam_host(C.byref(imp), arr, nj, _ptr(iq), int(sample0), n, int(fmt),
                              _ptr(out)))
    return out


def _echo_array(echo):
    """(ctypes array or None, count) of an iterable of Echo; the count is passed on as it is, so
    that the library refuses more than MAXECHO"""
    echo = list(echo or ())
    return ((Echo * len(echo))(*echo) if echo else None), len(echo)


def echo_make(fs_hz, prn, delay_m, atten_db, phase_deg=0.0, doppler_hz=0.0):
    """An Echo from physical parameters (gss_echo_make): of satellite prn (0: of every one), the
    extra path delay_m in metres, atten_db below the direct signal, its carrier phase_deg against
    the direct signal's at sample 0 and its own doppler_hz (fading) at the rate fs_hz."""
    e = Echo()
    _check(lib().gss_echo_make(float(fs_hz), int(prn), float(delay_m), float(atten_db),
                               float(phase_deg), float(doppler_hz), C.byref(e)))
    return e


def echo_host(echo, blk, nch, ca, nav, n_per_blk, sample0, iq):
    """gss_echo_host: the echoes `echo` (an iterable of Echo) of the rows blk [nblk][MAXCH], nch
    [nblk] (tables ca, nav) added to their SC16 render iq (int16, 2 * nblk * n_per_blk); returns
    a new array, iq is left as it is."""
    blk = np.ascontiguousarray(blk, CHAN_DTYPE)
    nch = np.ascontiguousarray(nch, np.int32)
    ca = np.ascontiguousarray(ca, np.uint32)
    nav = np.ascontiguousarray(nav, np.uint32)
    out = np.array(iq, np.int16).reshape(-1)
    nblk = len(nch)
    if blk.size != nblk * MAXCH or out.size != 2 * nblk * int(n_per_blk):
        raise ValueError("echo_host: blk, nch and iq do not describe the same blocks")
    arr, ne = _echo_array(echo)
    _check(lib().gss_echo_host(arr, ne, _ptr(blk), _ptr(nch), nblk, int(n_per_blk), _ptr(ca),
                               ca.size // CA_WORDS, _ptr(nav), nav.size // NAV_WORDS,
                               int(sample0), _ptr(out)))
    return out


def fir_make(fs_hz, bw_hz, n_taps=63):
    """A Fir from physical parameters (gss_fir_make): a Hamming-windowed sinc of two-sided width
    bw_hz at the rate fs_hz with n_taps taps (odd, 3..63); DC gain 1, delay (n_taps - 1) / 2."""
    f = Fir()
    _check(lib().gss_fir_make(float(fs_hz), float(bw_hz), int(n_taps), C.byref(f)))
    return f


def fir_check(fir):
    """gss_fir_check: raises GssError for a filter the calls refuse."""
    _check(lib().gss_fir_check(C.byref(fir)))


def fir_host(fir, iq, halo, fmt):
    """The filter on the host (gss_fir_host): iq int16[2 n] SC16 samples, halo the n_taps - 1
    samples before them (int16[2 (n_taps - 1)]) or None for zeros; returns the bytes of format
    fmt as uint8."""
    iq = np.ascontiguousarray(iq, np.int16).reshape(-1)
    n = len(iq) // 2
    if halo is not None:
        halo = np.ascontiguousarray(halo, np.int16).reshape(-1)
        if halo.size != 2 * max(fir.n_taps - 1, 0):
            raise ValueError("fir_host: the halo is n_taps - 1 samples")
        if halo.size == 0:
            halo = None
    out = np.zeros(impair_bytes(n, fmt) if fmt in (1, 8, 16) else 0, np.uint8)
    _check(lib().gss_fir_host(C.byref(fir), _ptr(iq), _ptr(halo), n, int(fmt), _ptr(out)))
    return out


def _acq_samples(acq, samples):
    x = np.ascontiguousarray(samples)
    if x.nbytes < acq.sample_bytes():
        raise ValueError(f"the search reads {acq.sample_bytes()} bytes, got {x.nbytes}")
    return x


def acquire_host(acq, samples, want_grid=False, threads=8):
    """The acquisition search on the host (gss_acquire_host) over samples (any array holding the
    format's bytes): (peaks ACQ_PEAK_DTYPE [n_prn], grid uint64 [n_prn, 2 K + 1, T] or None,
    resolved qshift)."""
    x = _acq_samples(acq, samples)
    _, T, _, _, P = acq.sizes()
    peaks = np.zeros(P, ACQ_PEAK_DTYPE)
    grid = np.zeros((P, 2 * acq.n_half + 1, T), np.uint64) if want_grid else None
    sh = C.c_int(0)
    _check(lib().gss_acquire_host(C.byref(acq), _ptr(x), _ptr(peaks), _ptr(grid), C.byref(sh),
                                  threads))
    return peaks, grid, sh.value


def acq_expect(row, fs, sample_in_block=0):
    """The labels of one channel row (a CHAN_DTYPE scalar) at a sample of its block
    (gss_acq_expect): dict(prn, tau [samples], doppler_hz, cn0_offset_db)."""
    r = np.ascontiguousarray(row, CHAN_DTYPE).reshape(1)
    t = _Truth()
    _check(lib().gss_acq_expect(_ptr(r), float(fs), int(sample_in_block), C.byref(t)))
    return {"prn": t.prn, "tau": t.tau, "doppler_hz": t.doppler_hz,
            "cn0_offset_db": t.cn0_offset_db}


def acq_threshold(n_coh, cells, pfa=1e-3):
    """the detection threshold on acq_ratio for a search of `cells` cells (gss_acq_threshold)"""
    return float(lib().gss_acq_threshold(int(n_coh), int(cells), float(pfa)))


def acq_ratio(peak):
    """peak over mean floor of one ACQ_PEAK_DTYPE entry"""
    return float(peak["peak"]) * float(peak["floor_cnt"]) / float(peak["floor_sum"])


def cn0_dbhz(peak, coh_ms=1):
    """C/N0 estimate [dB-Hz] of one ACQ_PEAK_DTYPE entry: 10 log10((ratio - 1) / coherent time);
    -inf for a peak not above its floor"""
    r = acq_ratio(peak)
    return float(10 * np.log10((r - 1) / (coh_ms * 1e-3))) if r > 1 else float("-inf")


def trk_jobs(acq, peaks, sample0, n_epoch):
    """TRK_JOB_DTYPE [len(peaks)]: the jobs that continue the peaks of a search that began at
    sample sample0 (gss_trk_job_from_peak)"""
    peaks = np.ascontiguousarray(peaks, ACQ_PEAK_DTYPE).reshape(-1)
    jobs = np.zeros(len(peaks), TRK_JOB_DTYPE)
    for i in range(len(peaks)):
        _check(lib().gss_trk_job_from_peak(C.byref(acq), _ptr(peaks[i:i + 1]), int(sample0),
                                           int(n_epoch), _ptr(jobs[i:i + 1])))
    return jobs


def _trk_args(trk, samples, n, jobs, pitch):
    x = np.ascontiguousarray(samples)
    cap = {FMT_SC16: x.nbytes // 4, FMT_SC08: x.nbytes // 2, FMT_SC01: x.nbytes * 4}.get(trk.fmt, 0)
    n = cap if n is None else int(n)
    if n > cap:
        raise ValueError(f"{n} samples asked for, the array holds {cap}")
    jobs = np.ascontiguousarray(jobs, TRK_JOB_DTYPE).reshape(-1)
    if pitch is None:
        pitch = max(int(jobs["n_epoch"].max()), 0) if len(jobs) else 0
    return x, n, jobs, int(pitch)


def track_host(trk, samples, jobs, n=None, pitch=None, threads=8):
    """Tracking on the host (gss_track_host) over samples (any array holding the format's bytes;
    n: how many of them, default all): (rec TRK_REC_DTYPE [n_job, pitch], count int32 [n_job])"""
    x, n, jobs, pitch = _trk_args(trk, samples, n, jobs, pitch)
    rec = np.zeros((len(jobs), pitch), TRK_REC_DTYPE)
    count = np.zeros(len(jobs), np.int32)
    _check(lib().gss_track_host(C.byref(trk), _ptr(x), n, _ptr(jobs), len(jobs), _ptr(rec), pitch,
                                _ptr(count), threads))
    return rec, count


def nav_decode(rec, skip=-1, cap=64):
    """The subframes in one job's records (gss_nav_decode): (NAV_SF_DTYPE [found], bit offset)"""
    rec = np.ascontiguousarray(rec, TRK_REC_DTYPE).reshape(-1)
    sf = np.zeros(cap, NAV_SF_DTYPE)
    off = C.c_int32(0)
    n = lib().gss_nav_decode(_ptr(rec), len(rec), int(skip), _ptr(sf), cap, C.byref(off))
    if n < 0:
        _check(n)
    return sf[:n].copy(), off.value


def trk_cn0(rec, skip=500):
    """tracked C/N0 [dB-Hz] of one job's records from epoch skip on (gss_trk_cn0)"""
    rec = np.ascontiguousarray(rec, TRK_REC_DTYPE).reshape(-1)
    return float(lib().gss_trk_cn0(_ptr(rec), len(rec), int(skip)))


def _obs_args(rec, count):
    rec = np.ascontiguousarray(rec, TRK_REC_DTYPE)
    if rec.ndim != 2:
        raise ValueError("rec must be [n_job, pitch]")
    count = np.ascontiguousarray(count, np.int32).reshape(-1)
    if len(count) != rec.shape[0]:
        raise ValueError("one count per job")
    return rec, count


def observables_host(fs_hz, rec, count, t_first, step, n_fix, threads=8):
    """gss_obs_host: OBS_DTYPE [n_job, n_fix], the code phase and accumulated carrier of every job
    (rec TRK_REC_DTYPE [n_job, pitch], count [n_job] as tracking returns them) at the samples
    t_first + k step, k < n_fix"""
    rec, count = _obs_args(rec, count)
    obs = np.zeros((len(count), max(int(n_fix), 0)), OBS_DTYPE)
    _check(lib().gss_obs_host(int(fs_hz), _ptr(rec), rec.shape[1], _ptr(count), len(count),
                              int(t_first), int(step), int(n_fix), _ptr(obs), threads))
    return obs


class NavData:
    """gss_navdata: ephemerides and Klobuchar coefficients per PRN, from a RINEX file
    (NavData(path)) or from decoded subframes alone (NavData())"""

    def __init__(self, rinex=None):
        self._h = C.c_void_p()
        if rinex is None:
            _check(lib().gss_navdata_open_empty(C.byref(self._h)))
        else:
            _check(lib().gss_navdata_open_rinex(C.byref(self._h), os.fsencode(rinex)))

    def add_subframe(self, prn, sf):
        """one NAV_SF_DTYPE element (nav_decode)"""
        sf = np.ascontiguousarray(sf, NAV_SF_DTYPE).reshape(1)
        _check(lib().gss_navdata_add_subframe(self._h, int(prn), _ptr(sf)))

    def get(self, prn):
        """{field: value} of NAVDATA_FIELDS for the ephemeris in use"""
        f = np.zeros(len(NAVDATA_FIELDS))
        _check(lib().gss_navdata_get(self._h, int(prn), _ptr(f), len(f)))
        return dict(zip(NAVDATA_FIELDS, (float(x) for x in f)))

    def range(self, prn, week, sec, xyz, no_iono=False):
        """gss_pvt_range: (pseudorange [m], its rate [m/s]) the fix's model gives"""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(3)
        out = np.zeros(2)
        _check(lib().gss_pvt_range(self._h, int(prn), int(week), float(sec), _ptr(xyz),
                                   int(bool(no_iono)), _ptr(out)))
        return float(out[0]), float(out[1])

    def close(self):
        if self._h:
            lib().gss_navdata_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pvt_solve(navdata, fs, t, sats, no_iono=False, week=0):
    """gss_pvt_solve: the PvtFix at sample t from sats (PVT_SAT_DTYPE: each satellite's
    observable at t, its PRN and the epoch and TOW count of one subframe of its job)"""
    sats = np.ascontiguousarray(sats, PVT_SAT_DTYPE).reshape(-1)
    fix = PvtFix()
    opts = _PvtOpts(int(bool(no_iono)), int(week))
    _check(lib().gss_pvt_solve(navdata._h, float(fs), int(t), _ptr(sats), len(sats),
                               C.byref(opts), C.byref(fix)))
    return fix


def lut():
    s = np.zeros(512, np.int32)
    c = np.zeros(512, np.int32)
    _check(lib().gss_lut(_ptr(s), _ptr(c)))
    return s, c


def linearize(blk, nch, nav, n_per_blk, threads=8, ca=None, anch=None):
    """(lin[nblk, 16] LIN_DTYPE, fast[nblk] int32): the certified integer lines of every block
    (gss_linearize); fast[b] == 1 where the fast path renders block b exactly.  ca: the C/A
    table the blocks' ca_tbl index (default: ca_table(), PRN 1..32).  anch: the chain's anchors
    (ANCHOR_DTYPE [nblk, 16], gss_linearize_ex): the same rows, shorter carrier walks."""
    blk = np.ascontiguousarray(blk, CHAN_DTYPE)
    nch = np.ascontiguousarray(nch, np.int32)
    nav = np.ascontiguousarray(nav, np.uint32)
    ca = np.ascontiguousarray(ca_table() if ca is None else ca, np.uint32)
    lin = np.zeros((len(nch), MAXCH), LIN_DTYPE)
    fast = np.zeros(len(nch), np.int32)
    if anch is None:
        _check(lib().gss_linearize(_ptr(blk), _ptr(nch), len(nch), n_per_blk, _ptr(ca), len(ca),
                                   _ptr(nav), len(nav), _ptr(lin), _ptr(fast), threads))
    else:
        anch = np.ascontiguousarray(anch, ANCHOR_DTYPE)
        assert anch.size == len(nch) * MAXCH
        _check(lib().gss_linearize_ex(_ptr(blk), _ptr(nch), len(nch), n_per_blk, _ptr(ca),
                                      len(ca), _ptr(nav), len(nav), _ptr(anch), _ptr(lin),
                                      _ptr(fast), threads))
    return lin, fast


def minmax_mod(n, m, a, s):
    """exact (min, max) of (a + p s) mod m over 0 <= p < n (the certificate's core)"""
    mn, mx = C.c_uint64(), C.c_uint64()
    lib().gss_minmax_mod(n, m, a, s, C.byref(mn), C.byref(mx))
    return mn.value, mx.value


def hits_mod(n, lgB, a0, st, w, cap=64, scan=False):
    """the proof's ambiguous samples (gss_hits_mod): list of p, or None if more than cap"""
    out = np.zeros(max(cap, 1), np.int64)
    k = lib().gss_hits_mod(n, lgB, a0, st, w, _ptr(out), cap, int(bool(scan)))
    if k == -2:
        raise ValueError("invalid hits_mod arguments")
    return None if k < 0 else [int(v) for v in out[:k]]


def first_below(n, m, a, s, w):
    """least p in [0, n) with (a + p s) mod m < w, or n (the proof's ambiguous-sample search)"""
    return lib().gss_first_below(n, m, a, s, w)


def carr_advance(carr, step, n):
    return lib().gss_carr_advance(carr, step, n)


def carr_advance_ck(carr, step, n):
    """(phase after n samples, the NCK checkpoints of the block)"""
    ck = np.zeros(NCK)
    end = lib().gss_carr_advance_ck(carr, step, n, _ptr(ck))
    return end, ck


def code_advance(code, step, n, icode, ibit, iword):
    a, b, c = C.c_int32(icode), C.c_int32(ibit), C.c_int32(iword)
    ph = lib().gss_code_advance(code, step, n, C.byref(a), C.byref(b), C.byref(c))
    return ph, a.value, b.value, c.value


class Scenario:
    """Host control plane: gpssim.c's main() around the sample loop (gss_scn_*)."""

    def __init__(self, nav_file, *, llh=None, xyz=None, motion_file=None, nmea=False,
                 samp_freq=2.6e6, data_format=16, duration=None, start=None,
                 time_overwrite=False, iono=True, verbose=False, quiet=True,
                 user_motion_size=3000, carrier="float"):
        if carrier not in ("float", "int"):
            raise ValueError(f"carrier must be 'float' or 'int', not {carrier!r}")
        self._keep = []
        o = _Opts()
        o.nav_file = self._s(nav_file)
        o.motion_file = self._s(motion_file) if motion_file else None
        o.nmea = int(bool(nmea))
        if xyz is not None:
            o.has_xyz = 1
            o.xyz[:] = list(map(float, xyz))
        if llh is not None:
            o.has_llh = 1
            o.llh[:] = list(map(float, llh))
        o.samp_freq = float(samp_freq)
        o.data_format = int(data_format)
        o.duration = -1.0 if duration is None else float(duration)
        if start is not None:
            o.has_start = 1
            o.start[:] = [int(v) for v in start[:5]] + [int(start[5])]
            o.start_sec = float(start[5])
            o.time_overwrite = int(bool(time_overwrite))
        o.iono_disable = 0 if iono else 1
        o.verbose = int(bool(verbose))
        o.user_motion_size = int(user_motion_size)
        o.quiet = int(bool(quiet))
        o.carrier_int = int(carrier == "int")      # FLOAT_CARR_PHASE off (gpssim.h:4)
        self._carrier_int = o.carrier_int
        self._h = C.c_void_p()
        _check(lib().gss_scn_open(C.byref(self._h), C.byref(o)))
        self._init_info()

    @classmethod
    def from_cli(cls, argv):
        """(Scenario, output path) from the reference's command line (gss_cli_parse: same
        options, defaults and error messages, gpssim.c:1650-1852).  Raises SystemExit(1) where
        the reference exits 1."""
        cli = _Cli()
        args = [b"gps-sdr-sim"] + [str(a).encode() for a in argv]
        arr = (C.c_char_p * len(args))(*args)
        if lib().gss_cli_parse(len(args), arr, C.byref(cli)):
            raise SystemExit(1)
        self = cls.__new__(cls)
        self._keep = [cli]
        self._carrier_int = cli.opt.carrier_int
        self._h = C.c_void_p()
        _check(lib().gss_scn_open(C.byref(self._h), C.byref(cli.opt)))
        self._init_info()
        if cli.has_impair:                             # --cn0 / --noise-sigma (Device.run(impair=))
            self.impair = Impair(cli.impair.sigma_q8, cli.impair.shift, cli.impair.seed)
        if cli.n_jam:                                  # --jam (Device.run(jam=))
            self.jam = [Jam.from_buffer_copy(cli.jam[i]) for i in range(cli.n_jam)]
        if cli.n_echo:                                 # --multipath (Device.run(echo=))
            self.echo = [Echo.from_buffer_copy(cli.echo[i]) for i in range(cli.n_echo)]
        if cli.has_fir:                                # --bandwidth (Device.run(fir=))
            self.fir = Fir.from_buffer_copy(cli.fir)
        return self, cli.out_file.decode()

    impair = None                # the command line's noise options (from_cli), else None
    jam = None                   # the command line's jammers (from_cli: a list of Jam), else None
    echo = None                  # the command line's echoes (from_cli: a list of Echo), else None
    fir = None                   # the command line's front-end filter (from_cli: a Fir), else None

    def _init_info(self):
        inf = _Info()
        _check(lib().gss_scn_info(self._h, C.byref(inf)))
        self.n_per_blk, self.n_blocks = inf.n_per_blk, inf.n_blocks
        self.data_format, self.samp_freq, self.delt = inf.data_format, inf.samp_freq, inf.delt
        self.start_week, self.start_sec = inf.week, inf.sec

    def position(self):
        """(next run block this handle produces, blocks whose rows it has produced)"""
        inf = _Info()
        _check(lib().gss_scn_info(self._h, C.byref(inf)))
        return inf.next_block, inf.rows_out

    def seek(self, block, threads=8):
        """Skip to run block `block` without producing the blocks before it (gss_scn_seek): only
        the 30 s updates are replayed.  The slot carriers are unknown until set_carrier()."""
        _check(lib().gss_scn_seek(self._h, int(block), threads))

    def carrier(self):
        """The planner's carrier phase per channel slot at the next block ([16] float64)."""
        c = np.zeros(MAXCH, np.float64)
        _check(lib().gss_scn_carrier(self._h, _ptr(c)))
        return c

    def set_carrier(self, carr):
        c = np.ascontiguousarray(carr, np.float64)
        assert c.shape == (MAXCH,)
        _check(lib().gss_scn_set_carrier(self._h, _ptr(c)))

    def next_deferred(self, max_blocks, threads=8):
        """Next batch without its carrier phases: (blk, nch, chain[nb, 16] CHAIN_DTYPE);
        carr_chain() fills blk["carr0"] once the slot carriers at the first block are known."""
        blk = np.zeros((max_blocks, MAXCH), CHAN_DTYPE)
        nch = np.zeros(max_blocks, np.int32)
        chain = np.zeros((max_blocks, MAXCH), CHAIN_DTYPE)
        nb = C.c_int(0)
        _check(lib().gss_scn_next_deferred(self._h, max_blocks, _ptr(blk), _ptr(nch),
                                           _ptr(chain), C.byref(nb), threads))
        n = nb.value
        return blk[:n].copy(), nch[:n].copy(), chain[:n].copy()

    @property
    def carrier_int(self):
        return bool(self._carrier_int)

    def _s(self, v):
        b = str(v).encode()
        self._keep.append(b)
        return b

    def next(self, max_blocks, threads=8, with_ck=False):
        """Next batch: (blk[nb, 16] CHAN_DTYPE, nch[nb] int32), plus the carrier checkpoints
        ck[nb, 16, NCK] float64 when with_ck (recorded by the planner's own carrier walk)."""
        blk = np.zeros((max_blocks, MAXCH), CHAN_DTYPE)
        nch = np.zeros(max_blocks, np.int32)
        ck = np.zeros((max_blocks, MAXCH, NCK), np.float64) if with_ck else None
        nb = C.c_int(0)
        _check(lib().gss_scn_next(self._h, max_blocks, _ptr(blk), _ptr(nch), _ptr(ck),
                                  C.byref(nb), threads))
        n = nb.value
        if with_ck:
            return blk[:n].copy(), nch[:n].copy(), ck[:n].copy()
        return blk[:n].copy(), nch[:n].copy()

    def all_blocks(self, batch=500, threads=8, with_ck=False):
        parts = []
        while True:
            r = self.next(batch, threads, with_ck)
            if len(r[1]) == 0:
                break
            parts.append(r)
        if not parts:
            empty = (np.zeros((0, MAXCH), CHAN_DTYPE), np.zeros(0, np.int32))
            return empty + ((np.zeros((0, MAXCH, NCK)),) if with_ck else ())
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))

    def nav_table(self):
        rows = C.POINTER(C.c_uint32)()
        n = C.c_int(0)
        _check(lib().gss_scn_nav_table(self._h, C.byref(rows), C.byref(n)))
        if n.value == 0:
            return np.zeros((1, NAV_WORDS), np.uint32)
        return np.ctypeslib.as_array(rows, shape=(n.value, NAV_WORDS)).copy()

    def nav_sources(self):
        """the rows' GPU-producer sources (NAV_SRC_DTYPE [n]), same order as nav_table()"""
        src = _P()
        n = C.c_int(0)
        _check(lib().gss_scn_nav_sources(self._h, C.byref(src), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, NAV_SRC_DTYPE)
        buf = (C.c_uint8 * (n.value * NAV_SRC_DTYPE.itemsize)).from_address(src.value)
        return np.frombuffer(buf, NAV_SRC_DTYPE).copy()

    def plan_seconds(self):
        return lib().gss_scn_plan_seconds(self._h)

    def close(self):
        if self._h:
            lib().gss_scn_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _chain_args(carr, blk, nch, chain, fill=True):
    """The chain calls' shared arguments as (carr, blk, nch, chain), contiguous and typed.  fill:
    the call advances carr[16] (a copy) and writes carr0 into blk itself, which must then be a
    contiguous CHAN_DTYPE array already."""
    if fill:
        c = np.array(carr, np.float64, copy=True)
        assert c.shape == (MAXCH,) and blk.flags.c_contiguous and blk.dtype == CHAN_DTYPE
    else:
        c, blk = np.ascontiguousarray(carr, np.float64), np.ascontiguousarray(blk)
    return c, blk, np.ascontiguousarray(nch, np.int32), np.ascontiguousarray(chain, CHAIN_DTYPE)


def _rows(a, dtype, n=None):
    """Per-row records (guesses, walks, links, records) as a contiguous array of n rows."""
    a = np.ascontiguousarray(a, dtype)
    assert n is None or a.size == n
    return a


def carr_chain(carr, blk, nch, chain, n_per_blk, carrier_int=False, with_ck=True, threads=8):
    """The carrier chain over deferred rows (gss_carr_chain): fills blk["carr0"] in place from
    carr[16] = the slot carriers at the first block; returns (carrier after the last block,
    checkpoints [nb, 16, NCK] or None)."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain)
    nb = len(nch)
    ck = np.zeros((nb, MAXCH, NCK), np.float64) if with_ck else None
    _check(lib().gss_carr_chain(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), nb, int(n_per_blk),
                                int(bool(carrier_int)), _ptr(ck), threads))
    return c, ck


def carr_chain_guess(carr, blk, nch, chain, n_per_blk, starts_only=False):
    """Each row's guesses (gss_carr_chain_guess): SPEC_IN_DTYPE [nb, 16].  starts_only: the
    starts alone (gss_carr_chain_starts), live rows with k = 0 for the walkers to complete."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain, fill=False)
    gi = np.zeros((len(nch), MAXCH), SPEC_IN_DTYPE)
    fn = lib().gss_carr_chain_starts if starts_only else lib().gss_carr_chain_guess
    _check(fn(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), len(nch), int(n_per_blk), _ptr(gi)))
    return gi


def carr_line_end(carr, blk, nch, chain, n_per_blk):
    """The slots' carriers after the batch by the lines of gss_carr_chain_starts (a prediction)."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain, fill=False)
    out = np.zeros(MAXCH, np.float64)
    _check(lib().gss_carr_line_end(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), len(nch),
                                   int(n_per_blk), _ptr(out)))
    return out


def spec_host(gi, n_per_blk, threads=8):
    """The speculative walk of every row's segments (gss_spec_host): SPEC_DTYPE rows.  Rows with
    k = 0 get their segment guesses first, written back into gi (a contiguous array)."""
    gi = _rows(gi, SPEC_IN_DTYPE).reshape(-1)
    spec = np.zeros(len(gi), SPEC_DTYPE)
    _check(lib().gss_spec_host(_ptr(gi), len(gi), int(n_per_blk), _ptr(spec), threads))
    return spec


def carr_chain_spec(carr, blk, nch, chain, n_per_blk, gi, spec, threads=8):
    """The carrier chain from the rows' speculative walks (gss_carr_chain_spec): fills
    blk["carr0"] in place; returns (carrier after the last block, blocks where the translation
    carried through)."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain)
    n = len(nch) * MAXCH
    gi, spec = _rows(gi, SPEC_IN_DTYPE, n), _rows(spec, SPEC_DTYPE, n)
    hit = C.c_int(0)
    _check(lib().gss_carr_chain_spec(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), len(nch),
                                     int(n_per_blk), _ptr(gi), _ptr(spec), threads,
                                     C.byref(hit)))
    return c, hit.value


def carr_chain_anchored(carr, blk, nch, chain, n_per_blk, gi, spec, threads=8):
    """carr_chain_spec, also returning the chain's anchors (gss_carr_chain_anchored):
    (end carriers, hits, ANCHOR_DTYPE [nb, 16])."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain)
    n = len(nch) * MAXCH
    gi, spec = _rows(gi, SPEC_IN_DTYPE, n), _rows(spec, SPEC_DTYPE, n)
    anch = np.zeros((len(nch), MAXCH), ANCHOR_DTYPE)
    hit = C.c_int(0)
    _check(lib().gss_carr_chain_anchored(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), len(nch),
                                         int(n_per_blk), _ptr(gi), _ptr(spec), threads,
                                         C.byref(hit), _ptr(anch)))
    return c, hit.value, anch


def carr_anchors(blk, nch, n_per_blk, gi, spec, threads=8):
    """The anchors of rows whose carr0 a chain has set (gss_carr_anchors): ANCHOR_DTYPE [nb, 16]."""
    blk = np.ascontiguousarray(blk, CHAN_DTYPE)
    nch = np.ascontiguousarray(nch, np.int32)
    n = len(nch) * MAXCH
    gi, spec = _rows(gi, SPEC_IN_DTYPE, n), _rows(spec, SPEC_DTYPE, n)
    anch = np.zeros((len(nch), MAXCH), ANCHOR_DTYPE)
    _check(lib().gss_carr_anchors(_ptr(blk), _ptr(nch), len(nch), int(n_per_blk), _ptr(gi),
                                  _ptr(spec), _ptr(anch), threads))
    return anch


def spec_records(gi, spec, n_per_blk, threads=8):
    """Each row's record (gss_spec_records; the previous row of its slot from gi["pad"]):
    SPEC_REC_DTYPE rows shaped like gi."""
    gi = _rows(gi, SPEC_IN_DTYPE)
    spec = _rows(spec, SPEC_DTYPE, gi.size)
    rec = np.zeros(gi.shape, SPEC_REC_DTYPE)
    _check(lib().gss_spec_records(_ptr(gi), _ptr(spec), gi.size, int(n_per_blk), _ptr(rec),
                                  threads))
    return rec


def carr_chain_records(carr, blk, nch, chain, n_per_blk, rec, threads=8):
    """The chain from the rows' records (gss_carr_chain_records): fills blk["carr0"] in place;
    returns (carrier after the last block, rows whose record held)."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain)
    rec = _rows(rec, SPEC_REC_DTYPE, len(nch) * MAXCH)
    hit = C.c_int(0)
    _check(lib().gss_carr_chain_records(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), len(nch),
                                        int(n_per_blk), _ptr(rec), threads, C.byref(hit)))
    return c, hit.value


def spec_links(nch, chain, n_per_blk, gi, spec, threads=8):
    """Each row's link from its slot's previous row (gss_spec_links): SPEC_LINK_DTYPE [nb, 16]."""
    nch = np.ascontiguousarray(nch, np.int32)
    chain = np.ascontiguousarray(chain, CHAIN_DTYPE)
    n = len(nch) * MAXCH
    gi, spec = _rows(gi, SPEC_IN_DTYPE, n), _rows(spec, SPEC_DTYPE, n)
    link = np.zeros((len(nch), MAXCH), SPEC_LINK_DTYPE)
    _check(lib().gss_spec_links(_ptr(nch), _ptr(chain), len(nch), int(n_per_blk), _ptr(gi),
                                _ptr(spec), _ptr(link), threads))
    return link


def carr_chain_linked(carr, blk, nch, chain, n_per_blk, gi, spec, link, threads=8):
    """carr_chain_spec's result with the rows' links (gss_carr_chain_linked): fills blk["carr0"]
    in place; returns (carrier after the last block, blocks where the translation held)."""
    c, blk, nch, chain = _chain_args(carr, blk, nch, chain)
    n = len(nch) * MAXCH
    gi, spec = _rows(gi, SPEC_IN_DTYPE, n), _rows(spec, SPEC_DTYPE, n)
    link = _rows(link, SPEC_LINK_DTYPE, n)
    hit = C.c_int(0)
    _check(lib().gss_carr_chain_linked(_ptr(c), _ptr(blk), _ptr(nch), _ptr(chain), len(nch),
                                       int(n_per_blk), _ptr(gi), _ptr(spec), _ptr(link), threads,
                                       C.byref(hit)))
    return c, hit.value


class Device:
    """One GPU (gss_dev_*).  synth_host() moves host arrays; synth_device() takes raw device
    pointers (e.g. torch tensors' data_ptr()) and is stream-ordered."""

    def __init__(self, ordinal=0):
        self._h = C.c_void_p()
        _check(lib().gss_dev_open(C.byref(self._h), int(ordinal)))

    def reserve(self, max_blocks, n_per_blk):
        _check(lib().gss_dev_reserve(self._h, max_blocks, n_per_blk))

    def synth_host(self, blk, nch, ca, nav, n_per_blk, fmt, want_carr_end=False, ck=None):
        """ck: optional carrier checkpoints [nblk, 16, NCK] (Scenario.next(with_ck=True))."""
        blk = np.ascontiguousarray(blk, CHAN_DTYPE)
        if ck is not None:
            ck = np.ascontiguousarray(ck, np.float64)
            assert ck.shape == (len(nch), MAXCH, NCK), ck.shape
        nch = np.ascontiguousarray(nch, np.int32)
        ca = np.ascontiguousarray(ca, np.uint32)
        nav = np.ascontiguousarray(nav, np.uint32)
        nblk = len(nch)
        out = np.empty(nblk * block_bytes(n_per_blk, fmt), np.uint8)
        cend = np.zeros((nblk, MAXCH), np.float64) if want_carr_end else None
        _check(lib().gss_synth_host(self._h, _ptr(blk), _ptr(nch), _ptr(ck), _ptr(ca), len(ca),
                                    _ptr(nav), len(nav), nblk, n_per_blk, fmt, _ptr(out),
                                    _ptr(cend)))
        return (out, cend) if want_carr_end else out

    def synth_device(self, blk_ptr, nch_ptr, nch_max, ca_ptr, n_ca, nav_ptr, n_nav, nblk,
                     n_per_blk, fmt, out_ptr, carr_end_ptr=0, status_ptr=0, stream=0, ck_ptr=0):
        _check(lib().gss_synth_device(self._h, blk_ptr, nch_ptr, nch_max, ck_ptr or None, ca_ptr,
                                      n_ca, nav_ptr,
                                      n_nav, nblk, n_per_blk, fmt, out_ptr,
                                      carr_end_ptr or None, status_ptr or None, stream or None))

    def ca_table_device(self, out_ptr, stream=0):
        """the C/A table built on the device (gss_ca_table_device) into out_ptr [32][CA_WORDS]"""
        _check(lib().gss_ca_table_device(self._h, out_ptr, stream or None))

    def nav_rows_device(self, src_ptr, first, n, rows_ptr, stream=0):
        """nav rows [first, first + n) from device sources (gss_nav_rows_device)"""
        _check(lib().gss_nav_rows_device(self._h, src_ptr, first, n, rows_ptr, stream or None))

    def synth_lin_device(self, blk_ptr, nch_ptr, nch_max, lin_ptr, fast_ptr, fb_ptr, n_fb, ca_ptr,
                         n_ca, nav_ptr, n_nav, nblk, n_per_blk, fmt, out_ptr, status_ptr=0,
                         stream=0, ck_ptr=0):
        """gss_synth_lin_device: the certified fast path for blocks with fast[b] == 1 and the
        exact path for the n_fb blocks listed at fb_ptr; device pointers, stream-ordered."""
        _check(lib().gss_synth_lin_device(self._h, blk_ptr, nch_ptr, nch_max, lin_ptr, fast_ptr,
                                          fb_ptr or None, n_fb, ck_ptr or None, ca_ptr, n_ca,
                                          nav_ptr, n_nav, nblk, n_per_blk, fmt, out_ptr,
                                          status_ptr or None, stream or None))

    def timing_lin(self):
        """(fast-path launches, their average ms) since the last timing_reset()"""
        n, t = C.c_int(), C.c_float()
        _check(lib().gss_dev_timing_lin(self._h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def anchor_device(self, set_, blk_ptr, nch_ptr, nch_max, nblk, n_per_blk, ck_ptr=0,
                      carr_end_ptr=0, stream=0):
        """Stage A of a batch into anchor set set_ (0/1), asynchronous on stream."""
        _check(lib().gss_anchor_device(self._h, set_, blk_ptr, nch_ptr, nch_max, ck_ptr or None,
                                       nblk, n_per_blk, carr_end_ptr or None, stream or None))

    def render_device(self, set_, blk_ptr, nch_ptr, nch_max, ca_ptr, n_ca, nav_ptr, n_nav, nblk,
                      n_per_blk, fmt, out_ptr, status_ptr=0, stream=0):
        """Stage B of a batch from anchor set set_, asynchronous on stream."""
        _check(lib().gss_render_device(self._h, set_, blk_ptr, nch_ptr, nch_max, ca_ptr, n_ca,
                                       nav_ptr, n_nav, nblk, n_per_blk, fmt, out_ptr,
                                       status_ptr or None, stream or None))

    def impair_device(self, imp, iq_ptr, sample0, n, fmt, out_ptr, stream=0):
        """gss_impair_device: the additive noise over n SC16 samples at device pointer iq_ptr
        (absolute index sample0 on), format fmt to out_ptr (== iq_ptr: SC16 only); async."""
        _check(lib().gss_impair_device(self._h, C.byref(imp), C.c_void_p(iq_ptr), int(sample0),
                                       int(n), int(fmt), C.c_void_p(out_ptr),
                                       C.c_void_p(stream or None)))

    def jam_device(self, imp, jam, iq_ptr, sample0, n, fmt, out_ptr, stream=0):
        """gss_jam_device: impair_device with the jammers `jam` (an iterable of Jam) added."""
        arr, nj = _jam_array(jam)
        _check(lib().gss_jam_device(self._h, C.byref(imp), arr, nj, C.c_void_p(iq_ptr),
                                    int(sample0), int(n), int(fmt), C.c_void_p(out_ptr),
                                    C.c_void_p(stream or None)))

    def echo_device(self, echo, blk_ptr, nch_ptr, nblk, n_per_blk, ca_ptr, n_ca, nav_ptr, n_nav,
                    sample0, iq_ptr, stream=0):
        """gss_echo_device: the echoes `echo` (an iterable of Echo) added in place to the SC16
        render at device pointer iq_ptr (nblk * n_per_blk samples) of the device rows blk_ptr,
        nch_ptr with the device tables ca_ptr, nav_ptr; asynchronous on stream."""
        arr, ne = _echo_array(echo)
        _check(lib().gss_echo_device(self._h, arr, ne, C.c_void_p(blk_ptr), C.c_void_p(nch_ptr),
                                     int(nblk), int(n_per_blk), C.c_void_p(ca_ptr), int(n_ca),
                                     C.c_void_p(nav_ptr), int(n_nav), int(sample0),
                                     C.c_void_p(iq_ptr), C.c_void_p(stream or None)))

    def fir_device(self, fir, iq_ptr, halo_ptr, n, fmt, out_ptr, stream=0):
        """gss_fir_device: the filter `fir` over n SC16 samples at device pointer iq_ptr, the
        n_taps - 1 samples before them at halo_ptr (0: zeros), format fmt to out_ptr (out of
        place); asynchronous on stream."""
        _check(lib().gss_fir_device(self._h, C.byref(fir), C.c_void_p(iq_ptr),
                                    C.c_void_p(halo_ptr or None), int(n), int(fmt),
                                    C.c_void_p(out_ptr), C.c_void_p(stream or None)))

    def acquire(self, acq, samples_ptr, peaks_ptr, grid_ptr=0, qshift_ptr=0, stream=0):
        """gss_acquire_device: the acquisition search over the samples at device pointer
        samples_ptr; peaks (n_prn x 32 bytes), the optional grid and resolved shift go to device
        pointers; async on stream."""
        _check(lib().gss_acquire_device(self._h, C.byref(acq), C.c_void_p(samples_ptr),
                                        C.c_void_p(peaks_ptr), C.c_void_p(grid_ptr or None),
                                        C.c_void_p(qshift_ptr or None),
                                        C.c_void_p(stream or None)))

    def acquire_from_host(self, acq, samples, want_grid=False):
        """gss_acquire: acquire() on host samples; returns what acquire_host() returns."""
        x = _acq_samples(acq, samples)
        _, T, _, _, P = acq.sizes()
        peaks = np.zeros(P, ACQ_PEAK_DTYPE)
        grid = np.zeros((P, 2 * acq.n_half + 1, T), np.uint64) if want_grid else None
        sh = C.c_int(0)
        _check(lib().gss_acquire(self._h, C.byref(acq), _ptr(x), _ptr(peaks), _ptr(grid),
                                 C.byref(sh)))
        return peaks, grid, sh.value

    def track(self, trk, samples_ptr, n, jobs, rec_ptr, pitch, count_ptr, stream=0):
        """gss_track_device: tracking over the n samples at device pointer samples_ptr; jobs a
        host TRK_JOB_DTYPE array, records [n_job, pitch] to rec_ptr and the epochs written per
        job to count_ptr (device pointers).  Asynchronous on stream."""
        jobs = np.ascontiguousarray(jobs, TRK_JOB_DTYPE).reshape(-1)
        _check(lib().gss_track_device(self._h, C.byref(trk), C.c_void_p(samples_ptr), int(n),
                                      _ptr(jobs), len(jobs), C.c_void_p(rec_ptr), int(pitch),
                                      C.c_void_p(count_ptr), C.c_void_p(stream)))

    def track_from_host(self, trk, samples, jobs, n=None, pitch=None):
        """gss_track: track() on host samples; returns what track_host() returns."""
        x, n, jobs, pitch = _trk_args(trk, samples, n, jobs, pitch)
        rec = np.zeros((len(jobs), pitch), TRK_REC_DTYPE)
        count = np.zeros(len(jobs), np.int32)
        _check(lib().gss_track(self._h, C.byref(trk), _ptr(x), n, _ptr(jobs), len(jobs),
                               _ptr(rec), pitch, _ptr(count)))
        return rec, count

    def observables(self, fs_hz, rec_ptr, pitch, count_ptr, n_job, t_first, step, n_fix, obs_ptr,
                    stream=0):
        """gss_obs_device: the observables of n_job jobs whose records [n_job, pitch] and counts
        lie at device pointers (as track() left them) to obs_ptr (n_job x n_fix x 32 bytes, a
        device pointer).  Asynchronous on stream."""
        _check(lib().gss_obs_device(self._h, int(fs_hz), C.c_void_p(rec_ptr or None), int(pitch),
                                    C.c_void_p(count_ptr), int(n_job), int(t_first), int(step),
                                    int(n_fix), C.c_void_p(obs_ptr or None),
                                    C.c_void_p(stream or None)))

    def observables_from_host(self, fs_hz, rec, count, t_first, step, n_fix):
        """gss_obs: observables() on host arrays; returns what observables_host() returns."""
        rec, count = _obs_args(rec, count)
        obs = np.zeros((len(count), max(int(n_fix), 0)), OBS_DTYPE)
        _check(lib().gss_obs(self._h, int(fs_hz), _ptr(rec), rec.shape[1], _ptr(count),
                             len(count), int(t_first), int(step), int(n_fix), _ptr(obs)))
        return obs

    def run(self, scn, sink, first_block=0, n_blocks=-1, batch=100, threads=8, impair=None,
            jam=None, echo=None, fir=None):
        """Stream blocks [first_block, first_block + n_blocks) of Scenario scn through gss_run;
        sink(memoryview, first_block, nblocks) gets each batch's bytes in run order (the view
        is valid only during the call).  An exception in sink stops the run and is re-raised.
        impair: an Impair (additive noise, gss_run_opts_t.impair), None: off.  jam: an iterable of
        Jam (gss_run_opts_t.jam), None: none; jammers need an impair (its shift; sigma_q8 0: no
        noise).  echo: an iterable of Echo (gss_run_opts_t.echo), None: none; echoes need an
        impair as jammers do.  fir: a Fir (gss_run_opts_t.fir), the front-end filter before the
        quantiser, None: none; it needs an impair too."""
        err = []

        def _sink(user, ptr, n, first, nb):
            try:
                sink(memoryview((C.c_char * n).from_address(ptr)).cast("B"), first, nb)
                return 0
            except BaseException as e:          # noqa: BLE001 — re-raised below
                err.append(e)
                return 1

        cb = SINK_FN(_sink)
        arr, nj = _jam_array(jam)
        earr, ne = _echo_array(echo)
        if impair is None and nj == 0 and ne == 0 and fir is None:
            rc = lib().gss_run(self._h, scn._h, first_block, n_blocks, batch, threads, cb, None)
        else:
            ro = _RunOpts(None, None, None, None, C.pointer(impair) if impair is not None else None,
                          arr, nj, earr, ne, C.pointer(fir) if fir is not None else None)
            rc = lib().gss_run_ex(self._h, scn._h, first_block, n_blocks, batch, threads, cb,
                                  None, C.byref(ro))
        if err:
            raise err[0]
        _check(rc)

    def timing_reset(self):
        _check(lib().gss_dev_timing(self._h, 1, None, None, None))

    def timing(self):
        """(Stage B launches, avg Stage A ms, avg Stage B ms) since the last reset."""
        n, a, b = C.c_int(), C.c_float(), C.c_float()
        _check(lib().gss_dev_timing(self._h, 0, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def linearize_device(self, blk_ptr, nch_ptr, nblk, n_per_blk, ca_ptr, n_ca, nav_ptr, n_nav,
                         lin_ptr, fast_ptr, stream=0, anch_ptr=None):
        """gss_linearize_device: the fast path's proofs on the GPU (device pointers, rows as
        gss_linearize's, async on stream); anch_ptr: the chain's anchors on the device
        (gss_linearize_device_ex)."""
        if anch_ptr is None:
            _check(lib().gss_linearize_device(self._h, C.c_void_p(blk_ptr), C.c_void_p(nch_ptr),
                                              nblk, n_per_blk, C.c_void_p(ca_ptr), n_ca,
                                              C.c_void_p(nav_ptr), n_nav, C.c_void_p(lin_ptr),
                                              C.c_void_p(fast_ptr), C.c_void_p(stream)))
        else:
            _check(lib().gss_linearize_device_ex(self._h, C.c_void_p(blk_ptr),
                                                 C.c_void_p(nch_ptr), nblk, n_per_blk,
                                                 C.c_void_p(ca_ptr), n_ca, C.c_void_p(nav_ptr),
                                                 n_nav, C.c_void_p(anch_ptr), C.c_void_p(lin_ptr),
                                                 C.c_void_p(fast_ptr), C.c_void_p(stream)))

    def spec_records_device(self, in_ptr, nrow, n_per_blk, d_in_ptr, d_spec_ptr, rec_ptr,
                            stream=0):
        """gss_spec_records_device: walks and records on the GPU (in / rec host-visible, d_in /
        d_spec device scratch of nrow rows), async on stream."""
        _check(lib().gss_spec_records_device(self._h, C.c_void_p(in_ptr), nrow, n_per_blk,
                                             C.c_void_p(d_in_ptr), C.c_void_p(d_spec_ptr),
                                             C.c_void_p(rec_ptr), C.c_void_p(stream)))

    def spec_device(self, in_ptr, nrow, n_per_blk, spec_ptr, stream=0):
        """gss_spec_device on raw device pointers (nrow SPEC_IN_DTYPE rows in, SPEC_DTYPE rows
        out), async on stream."""
        _check(lib().gss_spec_device(self._h, C.c_void_p(in_ptr), nrow, n_per_blk,
                                     C.c_void_p(spec_ptr), C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib().gss_dev_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
