/*
 * gpssim_amd.h — C ABI of the MI355X-native GPS L1 C/A baseband synthesiser.
 *
 * The reference (TheShinning/gps-sdr-sim) has no plugin/FFI API: its hot path is inline code in
 * main() (gpssim.c:2190-2288) operating on locals chan[MAX_CHAN], gain[], iq_buff, iq8_buff, delt,
 * iq_buff_size and data_format (gpssim.c:1686-1716).  The seam this library exports is therefore
 * "synthesise K consecutive 0.1 s blocks given per-block channel parameters" (SURVEY.md §8b), plus
 * the host control plane that produces those parameters (gpssim.c:1672-2353 minus the sample loop).
 *
 * Two layers, one shared library (libgpssim_amd.so):
 *   1. Device layer (gss_dev_*, gss_synth_*): the hot path.  Replaces the per-sample loop
 *      gpssim.c:2190-2264 and the quantise/pack epilogue gpssim.c:2257-2288.  Plain pointers and
 *      sizes only; results are stream-ordered on the caller's HIP stream.
 *   2. Host layer (gss_scn_*): ephemeris parsing, 10 Hz range/Doppler refresh, nav message and
 *      channel allocation, and the exact carrier-phase planner.  Replaces gpssim.c:1672-2188 and
 *      2290-2353 (everything in main() around the sample loop).
 *
 * Error convention: every entry point returns 0 on success and a negative GSS_E* code on failure;
 * gss_last_error() returns a human-readable message for the calling thread.  Nothing here calls
 * exit(); the CLI (gps-sdr-sim) turns a failure into the reference's fprintf(stderr,…); exit(1).
 * Threading: a gss_dev / gss_scn handle is not thread-safe; use one host thread per GPU.
 */
#ifndef GPSSIM_AMD_H
#define GPSSIM_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSS_MAXCH      16    /* MAX_CHAN, gpssim.h:16 */
#define GSS_CA_LEN     1023  /* CA_SEQ_LEN, gpssim.h:36 */
#define GSS_CA_WORDS   32    /* 1023 chips packed 32 per uint32 (bit j%32 of word j/32) */
#define GSS_NAV_WORDS  60    /* N_DWRD, gpssim.h:33 */

/* data formats: -b 1 / 8 / 16 (SC01/SC08/SC16, gpssim.h:77-79) */
#define GSS_FMT_SC01   1
#define GSS_FMT_SC08   8
#define GSS_FMT_SC16   16

#define GSS_OK           0
#define GSS_E_ARG       -1   /* invalid argument */
#define GSS_E_HIP       -2   /* HIP runtime error */
#define GSS_E_NOMEM     -3   /* allocation failed */
#define GSS_E_IO        -4   /* file open/read/write failed */
#define GSS_E_INPUT     -5   /* invalid input data (RINEX, motion file, start time …) */
#define GSS_E_STATE     -6   /* call out of order / exhausted */
#define GSS_E_NODEV     -7   /* no GPU / kernel image unavailable */
#define GSS_E_RANGE     -8   /* nav-word index ran past dwrd[59] (gpssim.c:2229-2232 overflow) */

/* ------------------------------------------------------------------------------------------ */
/* Per (block, channel) parameters: everything the sample loop reads.        */
/* ------------------------------------------------------------------------------------------ */
typedef struct gss_chan_blk {
    double  carr0;      /* chan[i].carr_phase at the block's first sample [cycles], FLOAT_CARR_PHASE
                           (gpssim.h:4).  Carried across blocks by the exact planner (gss_scn_*).   */
    double  carr_step;  /* chan[i].f_carr * delt, re-multiplied each sample in gpssim.c:2245       */
    double  code0;      /* chan[i].code_phase after computeCodePhase (gpssim.c:1334) [chips]       */
    double  code_step;  /* chan[i].f_code * delt (gpssim.c:2212)                                   */
    int32_t icode;      /* gpssim.c:1342 */
    int32_t ibit;       /* gpssim.c:1339 */
    int32_t iword;      /* gpssim.c:1336 */
    int32_t gain;       /* gain[i] (gpssim.c:2186), scaled by 2^7                                 */
    int32_t ca_tbl;     /* row of the ca_bits table (normally prn-1)                               */
    int32_t nav_tbl;    /* row of the dwrd table (chan[i].dwrd version)                            */
} gss_chan_blk_t;       /* 56 bytes; blocks are laid out [nblk][GSS_MAXCH], first nch[b] valid     */

/* ------------------------------------------------------------------------------------------ */
/* Device layer                                                                                */
/* ------------------------------------------------------------------------------------------ */
typedef struct gss_dev gss_dev;

/* Open device `ordinal` (hipSetDevice).  Fails with GSS_E_NODEV when no GPU is visible.       */
int gss_dev_open(gss_dev **out, int ordinal);
int gss_dev_close(gss_dev *d);

/* Pre-size both anchor sets for batches of up to `max_blocks` blocks of `n_per_blk` samples,
   so that the synthesis calls perform no allocation (graph-capturable).                       */
int gss_dev_reserve(gss_dev *d, int max_blocks, int n_per_blk);

/* Bytes of output one block produces: n*4 (SC16), n*2 (SC08), n/4 (SC01; n%4==0 required,
   see SURVEY.md Appendix A.4).  Returns 0 for an invalid format.                              */
size_t gss_block_bytes(int n_per_blk, int fmt);

/* Carrier checkpoints per block and channel: carr_ck[b][k][j] = exact carrier phase at sample
   (j * n_per_blk) / GSS_NCK of the block (j = 0 is carr0).  The host planner records them while
   it walks the carrier chain anyway (gss_scn_next); with them the GPU walks each block's carrier
   as GSS_NCK independent sub-chains.  Optional everywhere (NULL: the GPU walks whole blocks).   */
#define GSS_NCK 8

/* Synthesise nblk consecutive 0.1 s blocks.  ALL pointers are device pointers:
     blk      [nblk][GSS_MAXCH] channel parameters (first nch[b] of each row valid)
     nch      [nblk] active channel count per block (0..16)
     nch_max  host-side upper bound of nch[] over the batch (selects the kernel instance;
              blocks with fewer channels are padded with silent channels)
     carr_ck  optional [nblk][GSS_MAXCH][GSS_NCK] carrier checkpoints (see above)
     ca_bits  [n_ca][GSS_CA_WORDS] packed C/A chips (codegen, gpssim.c:132-171)
     nav      [n_nav][GSS_NAV_WORDS] 30-bit nav words (chan[i].dwrd, gpssim.c:1467-1547)
     out      nblk * gss_block_bytes(n_per_blk, fmt) bytes, exactly the bytes the reference
              fwrite()s for those blocks (gpssim.c:2276/2283/2287), concatenated in block order
     carr_end optional [nblk][GSS_MAXCH]: carrier phase after the block's last sample
     status   optional int32[1]: set non-zero if a nav-word index ran past 59 on any of a
              block's n_per_blk code-phase adds, the add of the block's last sample included
              (the reference counts the wrap in the sample that makes it, gpssim.c:2212-2237),
              or was past 59 in a row; never cleared (the caller zeroes it)
     out      needs no alignment (a misaligned base takes narrower stores)
     carr0    may be exactly 1.0 (what a descending wrap's + 1.0 can round to): the first step
              is then the reference's 1 + carr_step >= 1 -> - 1, also for carr_step == 0.
              carr0 + carr_step must stay below 2.0 in double arithmetic: the one row that does
              not, carr0 == 1.0 with carr_step == 1 - 2^-53, is unsupported here and refused by
              gss_synth_host (GSS_E_ARG)
   stream is a hipStream_t (NULL = default stream).  Asynchronous; no host synchronisation.    */
int gss_synth_device(gss_dev *d, const gss_chan_blk_t *blk, const int32_t *nch, int nch_max,
                     const double *carr_ck, const uint32_t *ca_bits, int n_ca, const uint32_t *nav, int n_nav,
                     int nblk, int n_per_blk, int fmt, void *out, double *carr_end,
                     int32_t *status, void *stream);

/* gss_synth_device in its two stages, for pipelining consecutive batches (Stage A of batch k+1
   on one stream while Stage B renders batch k on another).  Stage A writes the exact state at
   every segment start of the batch into anchor set `set` (0 or 1, device-owned buffers); Stage
   B renders from that set.  Arguments as gss_synth_device; the caller orders the two on its
   streams (events) and passes Stage B the same blk/nch/nch_max/nblk/n_per_blk as Stage A of
   that set.  gss_synth_device == gss_anchor_device(set 0) then gss_render_device(set 0) on one
   stream.                                                                                     */
int gss_anchor_device(gss_dev *d, int set, const gss_chan_blk_t *blk, const int32_t *nch,
                      int nch_max, const double *carr_ck, int nblk, int n_per_blk,
                      double *carr_end, void *stream);
int gss_render_device(gss_dev *d, int set, const gss_chan_blk_t *blk, const int32_t *nch,
                      int nch_max, const uint32_t *ca_bits, int n_ca, const uint32_t *nav,
                      int n_nav, int nblk, int n_per_blk, int fmt, void *out, int32_t *status,
                      void *stream);

/* ---- certified linear fast path ------------------------------------------------------------
   For most blocks each channel's exact carrier and code trajectories stay so close to a 64-bit
   integer line that every sample's LUT cell, chip and code wrap can be read off the line.
   gss_linearize (host) finds the lines and proves that, block by block, with exact integer
   arithmetic; gss_synth_lin_device renders the proven blocks with integer steps only and sends
   the rest (fast[b] == 0) through the exact walking path (Stage A + Stage B).  Same bytes.     */
#define GSS_NGC 8                /* signed-gain schedule entries per block and channel        */
#define GSS_NPATCH 8             /* patched samples per block and channel                     */
typedef struct gss_lin {
    uint64_t x0, xs;             /* carrier line, 2^-64 cycle: x0 + p*xs mod 2^64              */
    uint64_t z0, zs;             /* code line, 2^-50 chip, unwrapped: floor((z0 + p*zs) / 2^50)
                                    = chips since the block's code wrap base; chip index is that
                                    mod 1023 and the k-th code wrap falls where it reaches 1023k */
    int64_t pdelta[GSS_NPATCH];  /* correction of sample ppos[i]'s packed I/Q term (exact minus
                                    what the kernel's render arithmetic reads there, both
                                    gain * codeCA * (cos + 2^22 sin), gpssim.c:2190-2256)      */
    int32_t gpos[GSS_NGC];       /* gain*dataBit (gpssim.c:2186, 2234) is gval[i] for samples   */
    int32_t gval[GSS_NGC];       /* gpos[i] <= p < gpos[i+1]; gpos[0] = 0, unused = INT32_MAX   */
    int32_t ppos[GSS_NPATCH];    /* patched samples, ascending (unused = INT32_MAX)             */
} gss_lin_t;                     /* 192 bytes, laid out [nblk][GSS_MAXCH]                      */

/* Lines and proofs for nblk blocks (host arrays; ca_bits = [n_ca][GSS_CA_WORDS] and nav =
   [n_nav][GSS_NAV_WORDS] rows as passed to the synth calls).  fast[b] = 1 if every channel of
   block b is certified (and the block's gains fit the packed accumulator), else 0.  Runs on
   `threads` host threads.                                                                     */
int gss_linearize(const gss_chan_blk_t *blk, const int32_t *nch, int nblk, int n_per_blk,
                  const uint32_t *ca_bits, int n_ca, const uint32_t *nav, int n_nav,
                  gss_lin_t *lin, int32_t *fast, int threads);

/* gss_linearize on the GPU: the same proofs and the same rows, byte for byte (the per-channel
   proof is csrc/common/gss_proof.h on both sides).  Device pointers; asynchronous on `stream`.
   gss_run proves with this call the slots of its planner-bound runs (rows ahead, slots of >= 1024
   blocks: the -b 1 runs) and on the host threads the others; GSS_RUN_PROOF=gpu / host / split
   (every other slot on the GPU) forces a mode.  One workgroup per block; a small launch spreads
   the channels over waves (GSS_PROOF_STRIDE=4 / 16 / 32 forces the shape, for tests).    */
int gss_linearize_device(gss_dev *d, const gss_chan_blk_t *blk, const int32_t *nch, int nblk,
                         int n_per_blk, const uint32_t *ca_bits, int n_ca, const uint32_t *nav,
                         int n_nav, gss_lin_t *lin, int32_t *fast, void *stream);

/* gss_synth_device over the certified fast path.  Device pointers as gss_synth_device, plus
   lin [nblk][GSS_MAXCH] and fast [nblk] from gss_linearize, and the exact path's block list
   fb_list [n_fb] (device; the indices b with fast[b] == 0, n_fb known on the host).  carr_ck
   (optional) feeds the exact path's Stage A.  No carr_end output.                             */
int gss_synth_lin_device(gss_dev *d, const gss_chan_blk_t *blk, const int32_t *nch, int nch_max,
                         const gss_lin_t *lin, const int32_t *fast, const int32_t *fb_list,
                         int n_fb, const double *carr_ck, const uint32_t *ca_bits, int n_ca,
                         const uint32_t *nav, int n_nav, int nblk, int n_per_blk, int fmt,
                         void *out, int32_t *status, void *stream);

/* min and max of (a + p*s) mod m over 0 <= p < n, exactly (the certificate's core; exported for
   tests).                                                                                      */
void gss_minmax_mod(uint64_t n, uint64_t m, uint64_t a, uint64_t s, uint64_t *mn, uint64_t *mx);
/* tests: the least p in [0, n) with (a + p s) mod m < w (n if none; UINT64_MAX for m = 0 or
   m >= 2^62, w = 0 or w > m) -- the proof's enumeration of ambiguous samples */
uint64_t gss_first_below(uint64_t n, uint64_t m, uint64_t a, uint64_t s, uint64_t w);
/* the proof's ambiguous samples: p in [1, n) with (a0 + p st) mod 2^lgB < w, ascending, up to
   cap in hit[]; their number, -1 if more, -2 on bad arguments (scan: one descent per hit, else
   the three-gap stepping the proofs use; both give the same list; exported for tests)        */
int gss_hits_mod(uint64_t n, uint64_t lgB, uint64_t a0, uint64_t st, uint64_t w, int64_t *hit,
                 int cap, int scan);

/* Same, from host buffers: uploads inputs, runs, downloads `out` (and carr_end if non-NULL),
   synchronises.  Convenience for the CLI and tests; the bench uses gss_synth_device().
   Without carr_end it linearises and takes the fast path (env GSS_PATH=walk: exact path
   only).                                                                                      */
int gss_synth_host(gss_dev *d, const gss_chan_blk_t *blk, const int32_t *nch,
                   const double *carr_ck, const uint32_t *ca_bits, int n_ca, const uint32_t *nav, int n_nav,
                   int nblk, int n_per_blk, int fmt, void *out, double *carr_end);

/* ---- additive noise ---------------------------------------------------------------------------
   White Gaussian noise added to the 16-bit samples before the format's quantiser (an extension:
   the reference emits the noise-free sum of satellites).  Exact integer arithmetic, a function
   of the seed and the sample's absolute index in the run (run block * n_per_blk + position), so
   the bytes do not depend on how a run is cut into batches, windows or ranks.  For sample n
   with noise-free components x16 (as gpssim.c:2262-2263 stores them):
     words   w[0..3] = Philox4x32-10(counter {lo32(n >> 1), hi32(n >> 1), 0, 0}, key {lo32(seed),
             hi32(seed)}); I takes w[2 (n & 1)], Q takes w[2 (n & 1) + 1]
     normal  from a word u: sign = u >> 31, idx = (u >> 19) & 4095, f = (u >> 3) & 0xFFFF,
             mag = T[idx] + (((T[idx + 1] - T[idx]) * f) >> 16), T = gss_noise_table
     noise   g = (mag * sigma_q8 + 2^23) >> 24, negated if sign
     output  w = (x16 + g + ((1 << shift) >> 1)) >> shift (arithmetic); SC16 clamp(w, -32768,
             32767); SC08 clamp(w >> 4, -128, 127); SC01 bit = w > 0, packed as gpssim.c:2266-2276 */
typedef struct gss_impair {
    uint64_t seed;
    uint32_t sigma_q8;           /* noise sigma per component in 1/256 LSB of the 16-bit sample,
                                    <= 0x00FFFFFF                                              */
    int32_t  shift;              /* 0..8: common attenuation that makes room for the noise     */
} gss_impair_t;

/* T[4097], Q16: T[i] = round(65536 * Phi^-1(0.5 + i / 8192)) for i < 4096 and T[4096] =
   round(65536 * Phi^-1(1 - 1/32768)) = 262719 (4.009 sigma).                                  */
int gss_noise_table(int32_t *out);
/* The impairment of samples [sample0, sample0 + n) on the host: iq holds their 2 n noise-free
   int16 components, out receives n * 4 (SC16), n * 2 (SC08) or n / 4 (SC01; n % 4 == 0) bytes.
   out == iq is allowed for SC16 only.                                                         */
int gss_impair_host(const gss_impair_t *p, const int16_t *iq, uint64_t sample0, size_t n,
                    int fmt, void *out);
/* The same on the device: device pointers, asynchronous on stream.  The table is the handle's:
   gss_dev_open uploads it and gss_dev_close frees it.                                         */
int gss_impair_device(gss_dev *d, const gss_impair_t *p, const int16_t *iq, uint64_t sample0,
                      size_t n, int fmt, void *out, void *stream);

/* ---- jammers ----------------------------------------------------------------------------------
   Up to GSS_MAXJAM interferers added to the 16-bit samples beside the noise, before the format's
   quantiser (an extension): a tone, a linear sweep that repeats every P samples, either gated
   by a pulse.  Exact integer arithmetic mod 2^64, a function of the sample's absolute index n
   alone (the n of the noise), so the bytes do not depend on batches, windows or ranks:
     k = n div P,  m = n mod P
     PhiP = P step0 + rate (P (P - 1) / 2)                (the half taken before the product)
     Phi  = phase0 + k PhiP + m step0 + rate (m (m - 1) / 2)
     idx  = Phi >> 55                                      (0..511)
     on   = gate_period == 0 || ((n mod gate_period) + gate_shift) mod gate_period < gate_on
     jI = on ? (amp cos512[idx] + 2^15) >> 16 : 0          (arithmetic; tables of gss_lut)
     jQ = on ? (amp sin512[idx] + 2^15) >> 16 : 0
     output  w = (x16 + sum_j jI_j + g + ((1 << shift) >> 1)) >> shift  (Q alike with jQ)
   with g, the clamps and the packing of gss_impair_t above (sigma_q8 = 0: g is 0, a jammer
   without noise).  The phase is continuous across sweeps; rate = 0, P = 1 is a tone, Phi =
   phase0 + n step0.  Level: amp = 65536 writes the carrier table's 250, the amplitude of a
   satellite at gain 128 (the convention of --cn0): J/S = 0 dB against it, as power while the
   gate is on; amp <= 2^23 (42.1 dB) keeps amp 250 + 2^15 inside int32.                        */
#define GSS_MAXJAM 4
typedef struct gss_jam {
    uint64_t step0;        /* carrier step at the start of a sweep, 2^-64 cycle per sample (two's
                              complement)                                                      */
    uint64_t rate;         /* added to the step every sample, 2^-64 cycle per sample^2 (two's
                              complement); CW: 0                                               */
    uint64_t phase0;       /* phase of sample 0, 2^-64 cycle                                   */
    uint32_t sweep;        /* P >= 1: samples per sweep (CW: 1)                                */
    uint32_t amp;          /* 0..2^23: peak amplitude in 1/65536 of the carrier table's 250    */
    uint32_t gate_period;  /* 0: always on; else samples per pulse period                      */
    uint32_t gate_on;      /* 0..gate_period samples on                                        */
    uint32_t gate_shift;   /* 0..gate_period-1 (0 when gate_period is 0)                       */
    uint32_t pad;          /* 0                                                                */
} gss_jam_t;               /* 48 bytes */

/* A jammer from physical parameters, in IEEE double exactly as written here:
     step(f) = (int64) floor(f / fs_hz * 2^64 + 0.5)                     requires |f| < fs_hz / 2
     sweep_s == 0 (CW):  P = 1, rate = 0, step0 = step(f0_hz)            (f1_hz is not read)
     sweep_s > 0:        P = floor(sweep_s * fs_hz + 0.5) in 1..2^32-1, step0 = step(f0_hz),
                         rate = floor((step(f1_hz) - step(f0_hz)) / P)   (integers, floored)
     amp = floor(65536 * pow(10, js_db / 20) + 0.5) <= 2^23
     gate_period = floor(gate_period_s * fs_hz + 0.5) <= 2^32-1 (gate_period_s == 0: no gate),
     gate_on = floor(duty * gate_period + 0.5) with 0 <= duty <= 1, gate_shift = 0, phase0 = 0
   GSS_E_ARG for anything out of range (a gate_period_s > 0 that rounds to 0 included).        */
int gss_jam_make(double fs_hz, double js_db, double f0_hz, double f1_hz, double sweep_s,
                 double gate_period_s, double duty, gss_jam_t *out);
/* gss_impair_host with n_jam (0..GSS_MAXJAM) jammers added; p is required (its shift applies;
   sigma_q8 = 0: no noise); the buffer rules are gss_impair_host's; n_jam = 0: its bytes.
   GSS_E_ARG for a jammer with sweep = 0, amp > 2^23, gate_on > gate_period, gate_shift >=
   max(gate_period, 1) or pad != 0.                                                            */
int gss_jam_host(const gss_impair_t *p, const gss_jam_t *jam, int n_jam, const int16_t *iq,
                 uint64_t sample0, size_t n, int fmt, void *out);
/* The same on the device: device pointers, asynchronous on stream; jam is a host array, read
   before the call returns.                                                                    */
int gss_jam_device(gss_dev *d, const gss_impair_t *p, const gss_jam_t *jam, int n_jam,
                   const int16_t *iq, uint64_t sample0, size_t n, int fmt, void *out, void *stream);

/* ---- multipath echoes ----------------------------------------------------------------------------
   Up to GSS_MAXECHO specular echoes added to the 16-bit samples of a render, in place, before
   the impairment or the jammers (an extension): each a delayed, attenuated, phase-shifted copy
   of one satellite's signal (or of every satellite's), made from the channel rows the render
   itself read.  Exact integers, one statement for host, device and oracle
   (csrc/common/gss_echo.h).  Per block b and live pair (echo j, channel k < nch[b]; live: prn ==
   0 or prn == ca_tbl + 1, with 0 <= ca_tbl < n_ca and 0 <= nav_tbl < n_nav and the row's doubles
   in range, below), from the row:
     P0 = carr0 >= 1.0 ? 0 : (uint64)(carr0 * 2^64)            (carr0 in [0, 1])
     Ps = (uint64)(2 * (int64)trunc(carr_step * 2^63))
     C0 = (int64)floor(code0 * 2^32),  Cs = (int64)floor(code_step * 2^32 + 0.5)
     X0 = (((iword * 30 + ibit) * 20 + icode) * 1023) * 2^32 + C0 - delay        (int64)
     g  = clamp((gain * alpha_q16 + 2^15) >> 16, -32767, 32767)   (int64 product, arithmetic)
   and for sample s of the block, a = sample0 + b n + s its absolute index:
     X    = X0 + s Cs,  q = X >> 32 (arithmetic)
     chip = q mod 1023 (floored: 0..1022),  cp = max(q div 1023 (floored), 0)
     bit  = cp div 20,  word = min(bit div 30, 59),  pos = bit mod 30
     c    = bit (chip mod 32) of ca_bits[ca_tbl][chip div 32]        -> +-1
     d    = (nav[nav_tbl][word] >> (29 - pos)) & 1                   -> +-1
     Phi  = P0 + s Ps + theta0 + a dstep  (mod 2^64),  idx = Phi >> 55
     E_I += d c cos512[idx] g,  E_Q += d c sin512[idx] g     (int32; |E| < 2^30 by the clamp on g)
     y    = clamp_int16(x16 + ((E + 64) >> 7))                        for I and for Q
   (tables of gss_lut).  With delay 0, alpha_q16 65536 and theta0 = dstep = 0 an echo is the
   render's own term for that channel up to the Q32 rounding of the code step.  A delay that
   reaches before the row's frame (iword = ibit = icode = 0 and code0 < delay: X < 0) takes the
   periodic chip and the row's first data bit; that is a few microseconds per 30 s.  The index a
   is absolute, as for the noise and the jammers, so the bytes do not depend on batches, block
   ranges or ranks.
   Ranges.  A row is live only with 0 <= carr0 <= 1, -1 < carr_step < 1, 0 <= code0 < 1023 and
   0 <= code_step < 1024, where every conversion above is defined; any other row (a NaN or an
   infinity among them) adds nothing, on the host and on the device alike.  X is an int64 in two's
   complement: the chips counted from the frame's start, ((iword * 30 + ibit) * 20 + icode) * 1023
   + code0 + n_per_blk * code_step, must stay below 2^31 (a frame holds 36,828,000 and a 0.1 s
   block of the reference 102,300 more at any rate); beyond that X wraps and the chip and data
   bit with it.  The calls cannot check this on device rows and do not on host rows.           */
#define GSS_MAXECHO 4
typedef struct gss_echo {
    uint64_t delay;      /* code delay, 2^-32 chip; < 1023 * 2^32                              */
    uint64_t theta0;     /* carrier phase offset at absolute sample 0, 2^-64 cycle             */
    uint64_t dstep;      /* extra phase per sample (fading Doppler), 2^-64 cycle, mod 2^64     */
    uint32_t alpha_q16;  /* amplitude ratio to the direct signal, 65536 = 1; <= 4 * 65536      */
    int32_t  prn;        /* 1..32: rows with ca_tbl == prn - 1; 0: every channel               */
} gss_echo_t;            /* 32 bytes */

/* An echo from physical parameters, in IEEE double exactly as written here:
     delay     = (uint64) floor(delay_m * 1023000 / 299792458 * 2^32 + 0.5)   in [0, 1023 * 2^32)
     alpha_q16 = (uint32) floor(65536 * pow(10, -atten_db / 20) + 0.5)        <= 2^18
     theta0    = (uint64) ((t - floor(t)) * 2^64),  t = phase_deg / 360   (a product of 2^64: 0)
     dstep     = (uint64)(int64) floor(doppler_hz / fs_hz * 2^64 + 0.5)       |doppler_hz| < fs_hz / 2
   prn 0..32 (0: every channel).  GSS_E_ARG for anything out of range or not finite.           */
int gss_echo_make(double fs_hz, int prn, double delay_m, double atten_db, double phase_deg,
                  double doppler_hz, gss_echo_t *out);
/* The argument check of the calls below: GSS_E_ARG for n_echo outside 0..GSS_MAXECHO, a null
   array with n_echo > 0, delay >= 1023 * 2^32, alpha_q16 > 2^18, prn outside 0..32.           */
int gss_echo_check(const gss_echo_t *echo, int n_echo);
/* The echoes added in place to iq: nblk * n_per_blk SC16 pairs, the render of the rows blk
   [nblk][GSS_MAXCH], nch [nblk] with the tables ca_bits [n_ca][GSS_CA_WORDS] and nav [n_nav]
   [GSS_NAV_WORDS]; sample0 is the absolute index of block 0's first sample.  n_echo = 0, and a
   block with nch 0, leave the samples as they are.  GSS_E_ARG (nothing written) for invalid
   echoes, nch outside 0..GSS_MAXCH, n_ca or n_nav < 1, or a range that passes 2^64.           */
int gss_echo_host(const gss_echo_t *echo, int n_echo, const gss_chan_blk_t *blk,
                  const int32_t *nch, int nblk, int n_per_blk, const uint32_t *ca_bits, int n_ca,
                  const uint32_t *nav, int n_nav, uint64_t sample0, int16_t *iq);
/* The same on the device: blk, nch, ca_bits, nav and iq are device pointers (nch is not read by
   the host), echo is a host array read before the call returns; asynchronous on stream, no
   allocation.  GSS_ECHO_PATH=plain (read per call) takes the plain kernel: one sample per
   thread, straight from the definition and global memory.                                     */
int gss_echo_device(gss_dev *d, const gss_echo_t *echo, int n_echo, const gss_chan_blk_t *blk,
                    const int32_t *nch, int nblk, int n_per_blk, const uint32_t *ca_bits, int n_ca,
                    const uint32_t *nav, int n_nav, uint64_t sample0, int16_t *iq, void *stream);

/* ---- front-end band-limit filter ----------------------------------------------------------------
   A causal FIR filter with real taps over the 16-bit samples that the impairment or the jammers
   wrote (an extension: the IF filter in front of a receiver's ADC), applied before the
   quantiser.  Exact integers, one statement for host, device and oracle (csrc/common/gss_fir.h).
   The taps are Q14 (16384: a gain of 1).  For each component c (I or Q) of the SC16 input x and
   T = n_taps:
     acc[n] = sum_{k=0}^{T-1} taps[k] * x_c[n - k]          (int32)
     v      = (acc + 2^13) >> 14                             (arithmetic shift)
   and the output stage is the impairment's with w = v: SC16 clamp(v, -32768, 32767), SC08
   clamp(v >> 4, -128, 127), SC01 v > 0 in the reference's bit order.  x[n - k] for an index before
   the call's first sample comes from a halo, the T - 1 samples that precede in[0] (halo[T - 2] is
   x[-1]); a null halo stands for zeros, so a run's samples before absolute index 0 are zero.
   sum |taps[k]| <= 65535 makes |acc| <= 32768 * 65535 < 2^31: every sum is exact in int32 in any
   order, so packed 16-bit dot products agree bit for bit.                                      */
#define GSS_MAXTAP 64
typedef struct gss_fir {
    int32_t n_taps;            /* T: 1..GSS_MAXTAP                                              */
    int32_t pad;               /* 0                                                             */
    int16_t taps[GSS_MAXTAP];  /* Q14; taps[k] for k >= n_taps are not read                     */
} gss_fir_t;                   /* 136 bytes */

/* A Hamming-windowed sinc of two-sided width bw_hz at the rate fs_hz, in IEEE double exactly as
   written here:
     M = n_taps - 1,  c = bw_hz / fs_hz
     for k = 0..M:   m = k - M/2
                     s = (m == 0) ? c : sin(pi * c * m) / (pi * m)
                     d[k] = s * (0.54 - 0.46 * cos(2 * pi * k / M))
     S = d[0] + d[1] + ... (in index order)
     taps[k] = (int16) floor(d[k] / S * 16384 + 0.5);   taps[M/2] += 16384 - sum(taps)
   so the DC gain is exactly 1, the taps are symmetric and the group delay is M/2 samples.
   GSS_E_ARG for n_taps even or outside 3..63, bw_hz <= 0, bw_hz > fs_hz, or a non-finite
   argument.  bw_hz == fs_hz: a single tap of 16384 at the centre (a pure delay of M/2).       */
int gss_fir_make(double fs_hz, double bw_hz, int n_taps, gss_fir_t *out);
/* The argument check of the calls below: GSS_E_ARG for a null filter, n_taps outside
   1..GSS_MAXTAP, pad != 0, or sum |taps[k]| > 65535 over k < n_taps.                          */
int gss_fir_check(const gss_fir_t *fir);
/* The filter over n SC16 samples in (I, Q int16 pairs; 2-byte aligned) into format fmt at out:
   4 n, 2 n or n / 4 bytes (SC01: n a multiple of 4).  halo: the n_taps - 1 SC16 samples before
   in[0], or null for zeros.  Out of place: GSS_E_ARG (nothing written) when in and out overlap,
   and for an invalid filter, format or pointer.  Any n is accepted, n < n_taps - 1 too.       */
int gss_fir_host(const gss_fir_t *fir, const int16_t *in, const int16_t *halo, size_t n, int fmt,
                 void *out);
/* The same on the device: in, halo and out are device pointers, fir is a host struct read before
   the call returns; asynchronous on stream, no allocation.  GSS_FIR_PATH=plain (read per call)
   takes the plain kernel: one output per thread, straight from the definition and global
   memory.  The staged kernel needs in 4-byte aligned and some sample h < 16 at which in + 4 h and
   the output's byte of sample h are both 16-byte aligned (SC01: 4-byte); other pointers are
   accepted and give the same bytes at the plain kernel's speed.                                */
int gss_fir_device(gss_dev *d, const gss_fir_t *fir, const int16_t *in, const int16_t *halo,
                   size_t n, int fmt, void *out, void *stream);

/* ---- signal acquisition -------------------------------------------------------------------------
   A measurement of generated samples (an extension; the reference has no receiver): for every
   selected PRN a search over Doppler bins and code phases, the peak, and the noise floor around
   it.  Exact integer arithmetic up to the peak table (csrc/common/gss_acq.h):
     sizes    L = fs coh_ms / 1000 (floor) samples per coherent window, T = ceil(fs / 1000) code
              phases, N = n_coh L + T - 1 samples read, E = ceil(2 fs / 1023000) + 1
     wipe     bin k = -n_half..n_half, f_k = k bin_hz: step_k = floor((f_k 2^32 + fs / 2) / fs) mod
              2^32, idx = ((n step_k) mod 2^32) >> 23, (c, s) = (cos512, sin512)[idx] of gss_lut;
              yI = xI c + xQ s, yQ = xQ c - xI s
     quantise q = clamp((y + ((1 << sh) >> 1)) >> sh, -127, 127); sh = qshift, or for -1 the least
              sh >= 0 with (250 (max|xI| + max|xQ|)) >> sh <= 127 over the N samples
     replica  r_p[i] = +1 / -1 by chip (i 1023000 / fs) mod 1023 of row p - 1 of gss_ca_table
     power    P[p][k][tau] = sum_m (S_I^2 + S_Q^2) mod 2^64, S_c = sum_{i < L} q_c[tau + m L + i]
              r_p[m L + i], 0 <= tau < T
     peak     the maximum of P per PRN (ties: lowest k, then lowest tau); floor_sum / floor_cnt over
              the cells of the peak's bin farther than E from it (circular in T)               */
typedef struct gss_acq {
    int32_t  fs_hz;              /* sample rate [Hz]                                            */
    int32_t  fmt;                /* GSS_FMT_SC16 / SC08 / SC01: the file formats                */
    int32_t  coh_ms;             /* coherent window [ms], >= 1                                  */
    int32_t  n_coh;              /* M: windows summed non-coherently, 1..1000                   */
    int32_t  bin_hz;             /* Doppler bin width [Hz], > 0                                 */
    int32_t  n_half;             /* K: bins -K..K                                               */
    int32_t  qshift;             /* 0..24, or -1: auto                                          */
    uint32_t prn_mask;           /* bit p - 1 selects PRN p                                     */
} gss_acq_t;
typedef struct gss_acq_peak {
    uint64_t peak, floor_sum;
    uint32_t floor_cnt;
    int32_t  tau, bin, prn;      /* code phase [samples], bin index -K..K, PRN 1..32            */
} gss_acq_peak_t;                /* 32 bytes; one per selected PRN, ascending PRN               */
typedef struct gss_acq_truth {   /* what a channel row says the search should find              */
    double  tau;                 /* code phase [samples] in [0, 1023 / code_step)               */
    double  doppler_hz;
    double  cn0_offset_db;       /* 20 log10(gain / 128)                                        */
    int32_t prn, pad;
} gss_acq_truth_t;

/* The derived sizes (any pointer may be NULL); GSS_E_ARG for a search gss_acquire_* rejects:
   L > 2^20, n_coh > 1000, T <= 2 E + 1, an empty prn_mask, or a field out of its range.  A
   bin_hz above 500 / coh_ms leaves Doppler holes: accepted, with gss_last_error() set.        */
int gss_acq_sizes(const gss_acq_t *a, int32_t *L, int32_t *T, int64_t *N, int32_t *E,
                  int32_t *n_prn);
/* The search on the host (the reference statement): samples = N samples of a->fmt (SC01: from
   the MSB of the first byte), peaks [n_prn], grid NULL or [n_prn][2 K + 1][T], qshift_out NULL
   or the resolved shift.                                                                      */
int gss_acquire_host(const gss_acq_t *a, const void *samples, gss_acq_peak_t *peaks,
                     uint64_t *grid, int *qshift_out, int threads);
/* The same on the device: device pointers (d_grid, d_qshift may be NULL), asynchronous on stream,
   samples 2-byte aligned (SC08 / SC01: 1-byte).  Scratch (the wiped planes, the replicas and,
   without d_grid, the power rows) is kept per handle, grows on first use, synchronously, and is
   freed by gss_dev_close; one search per handle may be in flight.  GSS_ACQ_PATH=valu takes the
   plain integer correlator instead of the matrix cores (same outputs).                        */
int gss_acquire_device(gss_dev *d, const gss_acq_t *a, const void *d_samples,
                       gss_acq_peak_t *d_peaks, uint64_t *d_grid, int32_t *d_qshift,
                       void *stream);
/* gss_acquire_device from host buffers: uploads, searches, downloads, synchronises.           */
int gss_acquire(gss_dev *d, const gss_acq_t *a, const void *samples, gss_acq_peak_t *peaks,
                uint64_t *grid, int *qshift_out);
/* The labels of one channel row at sample `sample_in_block` of its block: code phase tau =
   ((1023 - code) / code_step) mod (1023 / code_step) with code = code0 + sample code_step,
   Doppler carr_step fs, and the level offset of its gain.                                     */
int gss_acq_expect(const gss_chan_blk_t *row, double fs, int64_t sample_in_block,
                   gss_acq_truth_t *out);
/* The detection threshold on ratio = peak floor_cnt / floor_sum: x / M where e^-x sum_{j < M}
   x^j / j! = pfa / cells (the maximum of `cells` noise-only cells of M summed windows exceeds it
   with probability about pfa).  NaN on bad arguments.                                         */
double gss_acq_threshold(int M, uint64_t cells, double pfa);

/* ---- signal tracking and LNAV decoding ----------------------------------------------------------
   What a receiver does after the search (an extension): per job one satellite's
   code and carrier are tracked over the samples, one record per code period, and the records'
   prompt sums are demodulated into navigation subframes.  The loops are an exact integer machine
   (csrc/common/gss_trk.h); host, device and tests/trk_oracle.py agree bit for bit on every record.
     constants  M = 1023 2^32 (code phase in 2^-32 chip), cs_nom = floor((1023000 2^32 + fs / 2) /
                fs); tables cos512 / sin512 of gss_lut; chips of row prn - 1 of gss_ca_table
     state      sample s = s0, code phase phi = 0, carrier phase th = 0 (uint32), carrier step
                w = w0 (int32, 2^-32 cycle per sample), W = w0 2^16 (int64), code step
                cs = cs_nom + w0 / 1540 (C's truncating division)
     epoch e    n = ceil((M - phi) / cs) samples; the job ends after n_epoch epochs or at the first
                epoch with s + n > N.  Sample i < n: c = phi + i cs; chips at c >> 32 (prompt),
                ((c + 2^31) mod M) >> 32 (early), ((c - 2^31) mod M) >> 32 (late), set -> +1, clear
                -> -1; carrier index ((th + i w) mod 2^32) >> 23; yI = xI cos + xQ sin, yQ = xQ cos
                - xI sin; IE, QE, IP, QP, IL, QL = sum y chip (int64)
     discrim.   amb(a, b) = max(|a|, |b|) + (min(|a|, |b|) >> 1); m = amb(IP, QP); u = IP 2^14 / m,
                v = QP 2^14 / m (truncating; 0 when m == 0); D_pll = u < 0 ? -v : v; D_fll = 0 in
                the job's first epoch, else with (u', v') of the epoch before cross = u' v - v' u,
                dot = u' u + v' v, D_fll = (dot < 0 ? -cross : cross) >> 14 (every >> floors);
                D_dll = (mE - mL) 2^14 / (mE + mL), mE = amb(IE, QE), mL = amb(IL, QL), 0 for 0 / 0
     update     th += n w; phi += n cs - M; s += n; e < n_pull: W += Kf D_fll, w = W >> 16; else
                W += Ki D_pll, w = (W + Kp D_pll) >> 16; W wraps mod 2^64 and w keeps the low 32
                bits; cs = cs_nom + w / 1540 + ((Kd D_dll) >> 16)
     limits     |w / 1540| <= 2^31 / 1540 and |(Kd D_dll) >> 16| <= Kd / 4 + 1 (|D_dll| <= 2^14), so
                with span = 2^31 / 1540 + Kd / 4 + 4 every cs lies inside cs_nom -+ span.  The calls
                reject a cfg with cs_nom - span <= M >> 23 (523,776) or cs_nom + span >= M: an
                epoch is then 1 <= n < 2^23 samples and no intermediate leaves int64            */
typedef struct gss_trk_cfg {
    int32_t fs_hz;               /* sample rate [Hz]                                            */
    int32_t fmt;                 /* GSS_FMT_SC16 / SC08 / SC01                                  */
    int32_t n_pull;              /* epochs of the frequency-locked pull-in, >= 0                */
    int32_t Kf, Ki, Kp, Kd;      /* loop gains, 0..2^30                                         */
} gss_trk_cfg_t;
typedef struct gss_trk_job {
    int64_t s0;                  /* sample where a code period starts, 0..2^62                  */
    int32_t prn;                 /* 1..32                                                       */
    int32_t w0;                  /* carrier step at the start [2^-32 cycle per sample]          */
    int32_t n_epoch;             /* epochs to track, 0..pitch                                   */
    int32_t pad;
} gss_trk_job_t;                 /* 24 bytes                                                    */
typedef struct gss_trk_rec {
    int64_t IE, QE, IP, QP, IL, QL;
    int64_t s;                   /* the epoch's first sample                                    */
    int32_t w;                   /* the carrier step the epoch used                             */
    int32_t dcs;                 /* the code step it used, minus cs_nom                         */
} gss_trk_rec_t;                 /* 64 bytes                                                    */
typedef struct gss_nav_sf {      /* one decoded subframe                                        */
    int64_t  sample;             /* first sample of its first epoch                             */
    int32_t  epoch;              /* index of that epoch's record                                */
    int32_t  polarity;           /* 1: the prompt sums were inverted                            */
    int32_t  tow, id;            /* TOW count and subframe id of the hand-over word             */
    uint32_t word[10];           /* the ten 30-bit words as transmitted                         */
} gss_nav_sf_t;                  /* 64 bytes                                                    */

/* The default loop: n_pull = 300 and, in double with T = 1e-3 and wn = 34 (an 18 Hz loop),
   Ki = round(wn^2 T 2^34 / (2 pi fs)), Kp = round(1.414 wn 2^34 / (2 pi fs)), Kf = round(0.05
   2^34 / (2 pi T fs)), Kd = round(8 2^33 / fs).  GSS_E_ARG for a cfg gss_track_* rejects.      */
int gss_trk_defaults(int32_t fs_hz, int32_t fmt, gss_trk_cfg_t *cfg);
/* The job that continues a peak of a search that began at sample `sample0`: s0 = sample0 + tau,
   w0 = the carrier step of the peak's bin.                                                     */
int gss_trk_job_from_peak(const gss_acq_t *a, const gss_acq_peak_t *peak, int64_t sample0,
                          int32_t n_epoch, gss_trk_job_t *job);
/* Tracking on the host (the reference statement): samples = N samples of cfg->fmt, rec
   [n_job][pitch], count [n_job] = the epochs written per job; jobs spread over threads.
   GSS_E_ARG for a cfg in which cs could fall to M / 2^23 (523,776: an epoch of 2^23 samples) or
   reach M (cs_nom -+ (2^31 / 1540 + Kd / 4 + 4)), a field out of its range, a PRN outside 1..32,
   s0 outside 0..2^62 or n_epoch outside 0..pitch.                                              */
int gss_track_host(const gss_trk_cfg_t *cfg, const void *samples, int64_t N,
                   const gss_trk_job_t *jobs, int n_job, gss_trk_rec_t *rec, int64_t pitch,
                   int32_t *count, int threads);
/* The same on the device: d_samples, d_rec (8-byte aligned) and d_count are device pointers,
   jobs is a host array (read before the call returns); asynchronous on stream.  A launch
   advances every job by at most 4096 epochs and leaves its state in device scratch (kept per
   handle, grown on first use, synchronously, freed by gss_dev_close; one call per handle may be
   in flight).
   GSS_TRK_PATH=plain takes the plain form of the kernel (same records).                        */
int gss_track_device(gss_dev *d, const gss_trk_cfg_t *cfg, const void *d_samples, int64_t N,
                     const gss_trk_job_t *jobs, int n_job, gss_trk_rec_t *d_rec, int64_t pitch,
                     int32_t *d_count, void *stream);
/* gss_track_device from host buffers: uploads, tracks, downloads, synchronises.                */
int gss_track(gss_dev *d, const gss_trk_cfg_t *cfg, const void *samples, int64_t N,
              const gss_trk_job_t *jobs, int n_job, gss_trk_rec_t *rec, int64_t pitch,
              int32_t *count);
/* LNAV subframes out of one job's n records.  Bit sync from epoch `skip` (< 0: 500): with nb =
   (n - skip - 19) / 20 bits per candidate, the offset o in 0..19 (to *bit_offset, may be NULL)
   that maximises sum_bits |sum_20 IP|, ties to the lowest; a bit is 1 when its 20-epoch sum of
   IP is >= 0.  Frame sync at every bit position with two bits before it (D29*, D30*), in both
   polarities: a subframe is accepted when its first eight bits are 10001011 and all ten words
   pass the IS-GPS-200 parity; the scan goes on behind it.  Returns the number of subframes
   written to sf[0 .. cap), or GSS_E_ARG.                                                       */
int gss_nav_decode(const gss_trk_rec_t *rec, int64_t n, int64_t skip, gss_nav_sf_t *sf, int cap,
                   int32_t *bit_offset);
/* Tracked C/N0 [dB-Hz] from the prompt powers P = IP^2 + QP^2 of records [skip, n) by their
   moments M2 = mean P, M4 = mean P^2: Pd = sqrt(2 M2^2 - M4), Pn = M2 - Pd, 10 log10(Pd / Pn /
   1e-3).  NaN when the moments leave no signal or fewer than two records remain.               */
double gss_trk_cn0(const gss_trk_rec_t *rec, int64_t n, int64_t skip);

/* ---- observables and position fixes ---------------------------------------------------------------
   What a receiver reads off its tracking loops (an extension).  A record stores
   neither the code phase nor the accumulated carrier; both follow exactly from a job's records
   by prefix sums (csrc/common/gss_obs.h; host, device and tests/obs_oracle.py agree bit for bit).
     lengths    n_e = s_(e+1) - s_e; the last record's is ceil((M - phi_e) / cs_e) as in tracking
                (0 when cs_e <= 0 or phi_e outside [0, M), which tracking never writes), with
                cs_e = cs_nom + dcs_e and M, cs_nom as above
     prefixes   phi_0 = 0, phi_(e+1) = phi_e + n_e cs_e - M;  A_0 = 0, A_(e+1) = A_e + n_e w_e.
                A is an int64 modulo 2^64 like W (so is phi, which tracking keeps below cs_e)
     instant    a sample index t inside epoch e, s_e <= t < s_e + n_e:
                code = phi_e + (t - s_e) cs_e   [2^-32 chip, below M]
                adr  = A_e + (t - s_e) w_e      [2^-32 cycle, modulo 2^64]
                epoch = e, w = w_e.  An instant before the job's first sample, at or past the end
                of its last epoch, or of a job without records: epoch = -1 and the rest 0
     instants   t_k = t_first + k step, k < n_fix
   The records' s must increase; the calls reject n_fix outside 0..2^30, |t_first| > 2^61,
   step < 1 and a last instant above 2^62.                                                      */
typedef struct gss_obs {
    int64_t code;                /* code phase at the instant [2^-32 chip]                      */
    int64_t adr;                 /* accumulated carrier since the job's start [2^-32 cycle]     */
    int32_t epoch;               /* the record the instant lies in, or -1                       */
    int32_t w;                   /* that record's carrier step                                  */
    int64_t pad;                 /* 0                                                           */
} gss_obs_t;                     /* 32 bytes                                                    */
/* rec [n_job][pitch] and count [n_job] as tracking left them (count[j] in 0..pitch), fs_hz the
   tracking's sample rate; obs [n_job][n_fix]; jobs spread over threads.                        */
int gss_obs_host(int32_t fs_hz, const gss_trk_rec_t *rec, int64_t pitch, const int32_t *count,
                 int n_job, int64_t t_first, int64_t step, int32_t n_fix, gss_obs_t *obs,
                 int threads);
/* The same on the device: d_rec (8-byte aligned), d_count and d_obs are device pointers, so the
   records need not leave the device between tracking and this; asynchronous on stream.  A count
   outside 0..pitch is clamped.  GSS_OBS_PATH=plain takes the plain form of the kernel (one lane
   walks a job; same bytes).                                                                    */
int gss_obs_device(gss_dev *d, int32_t fs_hz, const gss_trk_rec_t *d_rec, int64_t pitch,
                   const int32_t *d_count, int n_job, int64_t t_first, int64_t step,
                   int32_t n_fix, gss_obs_t *d_obs, void *stream);
/* gss_obs_device from host buffers: uploads, runs, downloads, synchronises.                    */
int gss_obs(gss_dev *d, int32_t fs_hz, const gss_trk_rec_t *rec, int64_t pitch,
            const int32_t *count, int n_job, int64_t t_first, int64_t step, int32_t n_fix,
            gss_obs_t *obs);

/* Navigation data: per PRN one ephemeris in use and the Klobuchar coefficients, from a RINEX
   file (every set is kept; a decoded subframe 2 or 3 selects the set with its IODE, and without
   one a fix takes the set whose clock epoch lies nearest) or from decoded subframes alone
   (subframes 1-3 with one IODE complete an ephemeris, scaled as IS-GPS-200 table 20-I and 20-III
   say; subframe 4 page 18 gives the ionosphere).                                               */
typedef struct gss_navdata gss_navdata;
int gss_navdata_open_rinex(gss_navdata **h, const char *path);
int gss_navdata_open_empty(gss_navdata **h);
/* 0, or GSS_E_ARG; a subframe that says nothing new (ids 4 and 5 but page 18) is accepted        */
int gss_navdata_add_subframe(gss_navdata *h, int prn, const gss_nav_sf_t *sf);
/* fields[0 .. n) of GSS_NAVDATA_FIELDS: 0 valid (0 / 1), 1 iode, 2 iodc, 3 toc [s], 4 toe [s],
   5 af0, 6 af1, 7 af2, 8 tgd, 9 crs, 10 deltan, 11 m0, 12 cuc, 13 ecc, 14 cus, 15 sqrta, 16 cic,
   17 omg0, 18 cis, 19 inc0, 20 crc, 21 aop, 22 omgdot, 23 idot (radians, not semicircles),
   24 ionosphere valid, 25..28 alpha, 29..32 beta, 33 week of toe (0 from subframes alone)       */
#define GSS_NAVDATA_FIELDS 34
int gss_navdata_get(const gss_navdata *h, int prn, double *fields, int n);
int gss_navdata_close(gss_navdata *h);

/* The fix.  Each satellite brings its observable at sample t and one anchor: the epoch and TOW
   count of any subframe decoded from the same job.  Its transmit time of week is
   6 (tow - 1) + (obs.epoch - sf_epoch) 1e-3 + obs.code / M 1e-3 seconds (the hand-over word
   counts the next subframe); the receive time is T0 + t / fs with T0, the GPS time of sample 0,
   unknown.  Iterated least squares over position and T0 in double on the host, against the
   simulator's own range model (orbit, clock polynomial with the relativistic term and tgd,
   flight-time and Sagnac rotation, Klobuchar; no troposphere), then velocity and clock drift
   from the Doppler w fs / 2^32 (sign as the carrier step of tracking).                         */
#define GSS_PVT_OK        0
#define GSS_PVT_FEW       1      /* fewer than four usable satellites                           */
#define GSS_PVT_SINGULAR  2      /* the geometry does not determine a fix                       */
#define GSS_PVT_DIVERGED  3      /* the iteration did not settle                                */
typedef struct gss_pvt_sat {
    gss_obs_t obs;               /* at sample t (epoch -1: the satellite is left out)           */
    int32_t prn;
    int32_t sf_epoch;            /* gss_nav_sf_t.epoch of the anchor                            */
    int32_t sf_tow;              /* its TOW count                                               */
    int32_t pad;
} gss_pvt_sat_t;                 /* 48 bytes                                                    */
typedef struct gss_pvt_opts {
    int32_t no_iono;             /* 1: the file was made without the ionosphere                 */
    int32_t week;                /* GPS week of the fix when the navdata does not hold one      */
} gss_pvt_opts_t;
typedef struct gss_pvt_fix {
    double xyz[3];               /* ECEF [m]                                                    */
    double llh[3];               /* latitude, longitude [rad], height [m]                       */
    double vel[3];               /* ECEF [m/s]                                                  */
    double t0_sec;               /* T0: seconds of week ...                                     */
    double t0_frac;              /* ... as t0_floor + t0_frac, t0_floor a whole second: the     */
    double t0_floor;             /*     fraction keeps what t0_sec rounds away                  */
    double drift;                /* receiver clock drift [s/s]                                  */
    double pdop;
    double rms;                  /* of the range residuals [m]                                  */
    int32_t t0_week;
    int32_t n_used;
    int32_t status;              /* GSS_PVT_*                                                   */
    int32_t iterations;
} gss_pvt_fix_t;                 /* 136 bytes                                                   */
/* 0 with out->status set (a fix that cannot be made is a status, not an error), or GSS_E_ARG.  */
int gss_pvt_solve(const gss_navdata *h, double fs, int64_t t, const gss_pvt_sat_t *sats, int n_sat,
                  const gss_pvt_opts_t *opts, gss_pvt_fix_t *out);
/* The model the fix inverts: out[0] the pseudorange [m] and out[1] its rate [m/s] of PRN prn at
   receive time (week, sec) and ECEF position xyz, with the handle's ephemeris in use.
   GSS_E_STATE when the handle holds none for the PRN.                                          */
int gss_pvt_range(const gss_navdata *h, int prn, int week, double sec, const double *xyz,
                  int no_iono, double *out);

/* Kernel timing from HIP events recorded on the launch stream around every Stage A and Stage B
   launch (gss_synth_device, gss_anchor_device, gss_render_device; rings of the last 256 of
   each).  reset!=0 clears the rings (no sync); otherwise waits for the last launches and
   returns the number n of Stage B launches and the average duration [ms] of each stage.      */
int gss_dev_timing(gss_dev *d, int reset, int *n, float *ckpt_ms, float *synth_ms);
/* Same for the fast-path kernel of gss_synth_lin_device (its exact-path leftovers count as
   Stage A / Stage B launches above); the same reset clears it.                               */
int gss_dev_timing_lin(gss_dev *d, int *n, float *lin_ms);

/* ------------------------------------------------------------------------------------------ */
/* Host layer: scenario driver mirroring main() (gpssim.c:1672-2353)                           */
/* ------------------------------------------------------------------------------------------ */
typedef struct gss_opts {
    const char *nav_file;       /* -e  RINEX v2 navigation file (required)                     */
    const char *motion_file;    /* -u  user motion CSV / -g NMEA GGA (NULL: static)            */
    int    nmea;                /* 1 if motion_file is NMEA GGA (-g)                           */
    int    has_xyz;             /* -c given: xyz holds ECEF [m]                                */
    double xyz[3];
    int    has_llh;             /* -l given: llh holds lat [deg], lon [deg], height [m]        */
    double llh[3];
    double samp_freq;           /* -s [Hz], default 2.6e6                                      */
    int    data_format;         /* -b 1/8/16, default 16                                       */
    double duration;            /* -d [s]; <0 → default USER_MOTION_SIZE/10                    */
    int    has_start;           /* -t / -T given                                               */
    int    time_overwrite;      /* -T                                                          */
    int    start[6];            /* y m d hh mm ss (already validated & floor()ed by caller)     */
    double start_sec;
    int    iono_disable;        /* -i                                                          */
    int    verbose;             /* -v                                                          */
    int    user_motion_size;    /* USER_MOTION_SIZE (gpssim.h:19-21), 0 → 3000                 */
    int    quiet;               /* suppress the reference's stderr chatter (library use)       */
    int    carrier_int;         /* 1: the reference built without FLOAT_CARR_PHASE (gpssim.h:4):
                                   32-bit integer carrier in 2^-25 cycle, step
                                   (int)round(2^25 f_carr delt) (gpssim.c:1623-1626, 2175-2177,
                                   2201-2202, 2252).  CLI: --carrier=int (default float).  The
                                   rows then carry that integer chain as exact doubles, carr0 =
                                   (carr_phase mod 2^25) / 2^25 and carr_step = step / 2^25, whose
                                   IEEE recurrence is the integer one, so every kernel renders it
                                   unchanged.                                                   */
} gss_opts_t;

/* The reference command line (getopt "e:u:g:c:l:o:s:b:T:t:d:iv", gpssim.c:1650-1852) parsed
   into options, with the reference's validation messages on stderr.  Returns 0 to run, 1 after
   printing usage or an error (the reference then exits with status 1).  The strings opt points
   at live in the struct.                                                                       */
typedef struct gss_cli {
    gss_opts_t opt;
    char nav_file[256], motion_file[256], out_file[256];
    /* extensions: --cn0=<dB-Hz> | --noise-sigma=<LSB>, --noise-shift=<0..8|auto>, --seed=<u64> */
    gss_impair_t impair;
    int has_impair;
    /* --jam=cw,<js_db>,<f_hz>[,pulse,<period_s>,<duty>] |
       --jam=sweep,<js_db>,<f0_hz>,<f1_hz>,<sweep_s>[,pulse,<period_s>,<duty>], up to GSS_MAXJAM
       times (gss_jam_make at the run's rate); sets has_impair (sigma_q8 = 0 without noise)    */
    gss_jam_t jam[GSS_MAXJAM];
    int n_jam;
    /* --multipath=<prn|all>,<delay_m>,<atten_db>[,<phase_deg>[,<doppler_hz>]], up to GSS_MAXECHO
       times (gss_echo_make at the run's rate); sets has_impair (sigma_q8 = 0 without noise)   */
    gss_echo_t echo[GSS_MAXECHO];
    int n_echo;
    /* --bandwidth=<hz>[,<taps>] (63 taps by default), once: gss_fir_make at the run's rate; sets
       has_impair (sigma_q8 = 0 without noise)                                                 */
    gss_fir_t fir;
    int has_fir;
} gss_cli_t;
int gss_cli_parse(int argc, char **argv, gss_cli_t *cli);
void gss_cli_usage(void);

typedef struct gss_scn_info {
    int    n_per_blk;           /* iq_buff_size = floor(fs/10) (gpssim.c:1877-1878)            */
    int    n_blocks;            /* numd-1: blocks the run writes (gpssim.c:2154)               */
    int    data_format;
    double samp_freq;           /* after rounding to a multiple of 10 Hz                       */
    double delt;                /* 1/samp_freq (gpssim.c:1881)                                 */
    int    week;  double sec;   /* g0 (start time)                                             */
    int64_t next_block;         /* run index of the next block gss_scn_next* produces          */
    int64_t rows_out;           /* blocks whose rows this handle produced (gss_scn_seek skips
                                   blocks without producing them)                              */
    int    carrier_int;         /* gss_opts_t.carrier_int                                      */
} gss_scn_info_t;

typedef struct gss_scn gss_scn;

/* Parse inputs, select ephemeris set and start time, allocate the first channels.
   On error returns GSS_E_* and *out stays NULL (message via gss_last_error()).               */
int gss_scn_open(gss_scn **out, const gss_opts_t *opt);
int gss_scn_info(const gss_scn *s, gss_scn_info_t *info);

/* Produce parameters for the next up to `max_blocks` blocks (in run order), including the
   exact carrier phase at each block start (planner runs on `threads` host threads).
   blk is [max_blocks][GSS_MAXCH], nch is [max_blocks], carr_ck (optional, may be NULL) is
   [max_blocks][GSS_MAXCH][GSS_NCK] carrier checkpoints.  *n_out = blocks produced (0 at end). */
int gss_scn_next(gss_scn *s, int max_blocks, gss_chan_blk_t *blk, int32_t *nch, double *carr_ck,
                 int *n_out, int threads);

/* ---- planning a time window without its prefix (multi-GPU: plan once, scatter) ----------------
   The carrier phase is the only state the sample loop carries across blocks (gpssim.c:2245-2250;
   the code state is recomputed every block, gpssim.c:1331-1345), and it is one chain per channel
   slot, restarted where allocateChannel re-initialises the slot (gpssim.c:1615-1626).  So a rank
   can produce its window's rows by itself (gss_scn_seek + gss_scn_next_deferred) and receive only
   the 16 slot carriers at its first block from the rank before it, which runs the chain over its
   own window (gss_carr_chain) and hands the end state on.                                     */
typedef struct gss_chain {       /* per (block, channel row): the carrier chain it continues     */
    int8_t  slot;                /* chan[] slot 0..15; -1 for padding rows                        */
    uint8_t reset;               /* 1: the slot's chain restarts at this block with `init`        */
    uint8_t pad[6];
    double  init;                /* carr_phase set by allocateChannel (valid when reset)          */
} gss_chain_t;                   /* 16 bytes, laid out [nblk][GSS_MAXCH] like the rows             */

/* gss_scn_next without the carrier chain: blk[].carr0 is left 0 and chain[] says which slot's
   chain each row continues; gss_carr_chain fills carr0 (and checkpoints) afterwards.  The
   handle's slot carriers (gss_scn_carrier) stay those at the first produced block, and
   gss_scn_next fails with GSS_E_STATE until gss_scn_set_carrier supplies the chain's end.       */
int gss_scn_next_deferred(gss_scn *s, int max_blocks, gss_chan_blk_t *blk, int32_t *nch,
                          gss_chain_t *chain, int *n_out, int threads);
/* The carrier chain over nblk consecutive blocks of deferred rows: carr[GSS_MAXCH] holds each
   slot's carrier phase at the first block's start on entry and after the last block on return;
   fills blk[].carr0 and, if carr_ck != NULL, the [nblk][GSS_MAXCH][GSS_NCK] checkpoints.
   carrier_int: the integer-carrier chain of gss_opts_t.carrier_int.  One slot per thread.    */
int gss_carr_chain(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                   const gss_chain_t *chain, int nblk, int n_per_blk, int carrier_int,
                   double *carr_ck, int threads);
/* The same chain with the blocks' walks run ahead of it, in parallel (the chain's serial part is
   then one partial cycle per block; gss_phase.h, "speculative block walk").
     gss_carr_chain_guess  each row's guesses: its start from the line of its slot (exact at the
                           slot's first block and at a reset) and up to GSS_SPEC_K - 1 segment
                           starts at wraps the line predicts, in[nblk][GSS_MAXCH] (padding: s 0)
     gss_carr_chain_starts the starts only, live rows left with k = 0: the walkers guess their
                           segment starts themselves and write them back into in[] (gss_run)
     gss_spec_host/device  the speculative walk of every row's segments: spec[nrow]; host
                           threads, or the GPU (device-visible pointers, async on stream; gss_run;
                           one lane per segment, rows channel-major for a multiple of GSS_MAXCH)
     gss_carr_chain_spec   the chain: as gss_carr_chain without checkpoints, each block's end from
                           its true start and its speculative walk (exact whether or not the
                           translation applies); *n_hit counts the blocks where it did.        */
#ifndef GSS_SPEC_T_DEFINED
#define GSS_SPEC_T_DEFINED
#ifndef GSS_SPEC_K
#define GSS_SPEC_K 32                   /* segments per block (8 before round 6: the GPU walks
                                          then took 1.19 ms per headline window, 0.88 with 16;
                                          with the row-shared cycle cache 0.65 with 16, 0.55
                                          with 32, 0.61 with 64: profiles/round6/spec_k/s6z) */
#endif
typedef struct gss_spec_in {           /* a row's guesses (host, gss_carr_chain_guess)          */
    double g, s;                       /* start guess, carr_step (0: padding row)               */
    int32_t k, pad;                    /* segments (1..GSS_SPEC_K; 0: not guessed yet)          */
    int64_t P[GSS_SPEC_K];             /* segment j >= 1 starts at sample P[j], a predicted wrap */
    double W[GSS_SPEC_K];              /* ... with post-wrap value W[j]                         */
} gss_spec_in_t;                       /* 24 + 16 GSS_SPEC_K bytes (536) */
typedef struct gss_spec_seg {
    double end, dlo, dhi;              /* end value, admissible translations of the start       */
    int64_t wrap_end;                  /* 1: the segment's last step wrapped                    */
} gss_spec_seg_t;
typedef struct gss_spec {              /* a row's speculative walk (GPU or host)                */
    int64_t p1;                        /* samples to the guess's first wrap (n: none)           */
    double w1;                         /* its post-wrap value                                   */
    gss_spec_seg_t seg[GSS_SPEC_K];
} gss_spec_t;                          /* 16 + 32 GSS_SPEC_K bytes (1040) */
#endif
int gss_carr_chain_guess(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                         const gss_chain_t *chain, int nblk, int n_per_blk, gss_spec_in_t *in);
int gss_carr_chain_starts(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                          const gss_chain_t *chain, int nblk, int n_per_blk, gss_spec_in_t *in);
/* The slots' carriers after the nblk blocks by the same lines: a prediction, the start of the
   next batch's guesses while this batch's chain is still pending (gss_run keeps two batches of
   walks in flight). */
int gss_carr_line_end(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                      const gss_chain_t *chain, int nblk, int n_per_blk, double *carr_end);
int gss_spec_host(gss_spec_in_t *in, int nrow, int n_per_blk, gss_spec_t *spec, int threads);
int gss_spec_device(gss_dev *d, gss_spec_in_t *in, int nrow, int n_per_blk, gss_spec_t *spec,
                    void *stream);
int gss_carr_chain_spec(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                        const gss_chain_t *chain, int nblk, int n_per_blk,
                        const gss_spec_in_t *in, const gss_spec_t *spec, int threads,
                        int *n_hit);
/* Records: each row's speculative walk folded into 72 bytes (gss_spec_rec_t: the interval of
   translations of its first post-wrap value that carry it through every segment, and of its
   predecessor's last translation that carry it from the predecessor's end), so that the chain
   needs neither the walks (1,040 B) nor the segment guesses (536 B) on the host (gss_run: the
   walks stay on the device and only the records cross the link).  The previous row of a row's
   slot chain in the batch is in[].pad (gss_carr_chain_starts / _guess set it; -1: none).
     gss_spec_records         the records from walks on the host
     gss_spec_records_device  walks and records on the GPU: in (host-visible rows, their
                              starts), d_in / d_spec (device scratch, nrow rows), rec
                              (host-visible); async on stream
     gss_carr_chain_records   the chain from the records (exact: a failed interval walks)   */
#ifndef GSS_SPEC_REC_DEFINED
#define GSS_SPEC_REC_DEFINED
typedef struct gss_spec_rec {
    double w1;                         /* post-wrap value at the guess's first wrap                */
    double slo, shi, sdd;              /* self: d0 = (true post-wrap value at p1) - w1 in [slo,
                                          shi] -> the row's last translation is d0 + sdd ...     */
    double end;                        /* ... and its end is end + (d0 + sdd)                      */
    double llo, lhi, ldd;              /* link: the previous row of the slot translated by d in
                                          [llo, lhi] -> this one's last translation is d + ldd    */
    int32_t p1;                        /* samples to the guess's first wrap                        */
    int32_t ok;                        /* bit 0: self record, bit 1: link record, bits 2..: the
                                          link's row distance (this row - in[].pad), which the
                                          chain checks against the slot's actual previous row  */
} gss_spec_rec_t;                      /* 72 bytes */
#endif
int gss_spec_records(const gss_spec_in_t *in, const gss_spec_t *spec, int nrow, int n_per_blk,
                     gss_spec_rec_t *rec, int threads);
int gss_spec_records_device(gss_dev *d, const gss_spec_in_t *in, int nrow, int n_per_blk,
                            gss_spec_in_t *d_in, gss_spec_t *d_spec, gss_spec_rec_t *rec,
                            void *stream);
int gss_carr_chain_records(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                           const gss_chain_t *chain, int nblk, int n_per_blk,
                           const gss_spec_rec_t *rec, int threads, int *n_hit);
/* Anchors: exact carrier values inside a block, by-products of the chain (the values at the
   segment starts its fix-up passed or walked), which the proofs start their exact carrier walks
   from (gss_linearize_ex / gss_linearize_device_ex) instead of from the block start.
     gss_carr_chain_anchored  gss_carr_chain_spec, also filling anch[nblk][GSS_MAXCH]
     gss_carr_anchors         the same anchors for rows whose carr0 any chain has set, in parallel
                              over blocks (the speculative walks of those rows, gss_spec_*)   */
typedef struct gss_carr_anchor {
    int32_t pos[GSS_SPEC_K];           /* sample positions within the block (-1: none); pos[0] 0 */
    double val[GSS_SPEC_K];            /* the reference's carr_phase at sample pos (val[0] carr0) */
} gss_carr_anchor_t;                   /* 12 GSS_SPEC_K bytes (384) */
int gss_carr_chain_anchored(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                            const gss_chain_t *chain, int nblk, int n_per_blk,
                            const gss_spec_in_t *in, const gss_spec_t *spec, int threads,
                            int *n_hit, gss_carr_anchor_t *anch);
int gss_carr_anchors(const gss_chan_blk_t *blk, const int32_t *nch, int nblk, int n_per_blk,
                     const gss_spec_in_t *in, const gss_spec_t *spec, gss_carr_anchor_t *anch,
                     int threads);
/* gss_linearize / gss_linearize_device with the anchors (anch [nblk][GSS_MAXCH], NULL: none;
   device memory for the _device form): the same rows, byte for byte, with shorter walks.      */
int gss_linearize_ex(const gss_chan_blk_t *blk, const int32_t *nch, int nblk, int n_per_blk,
                     const uint32_t *ca_bits, int n_ca, const uint32_t *nav, int n_nav,
                     const gss_carr_anchor_t *anch, gss_lin_t *lin, int32_t *fast, int threads);
int gss_linearize_device_ex(gss_dev *d, const gss_chan_blk_t *blk, const int32_t *nch, int nblk,
                            int n_per_blk, const uint32_t *ca_bits, int n_ca,
                            const uint32_t *nav, int n_nav, const gss_carr_anchor_t *anch,
                            gss_lin_t *lin, int32_t *fast, void *stream);
/* Links between a slot's consecutive rows, computed before the chain's start is known (the
   multi-rank planner runs them ahead of the baton; gpssim_amd/shard.py chain_speculated):
     gss_spec_links         for every row that continues its slot's chain in the batch, its
                            whole walk folded into one record from the previous row's
                            speculative end (its partial cycle to the first wrap walked from
                            there ahead of time, with the admissible translations)
     gss_carr_chain_linked  gss_carr_chain_spec's result, where a row whose predecessor's
                            translation held is one compare and two adds: the serial part is then
                            a few ns per row, plus the exact walks where a translation fails. */
typedef struct gss_spec_link {
    double lo, hi;                     /* the previous row translated by d in [lo, hi] (lo > hi:
                                          no record): this row translates too ...               */
    double dd, end;                    /* ... by d + dd, and ends at end + (d + dd)             */
} gss_spec_link_t;                     /* 32 bytes */
int gss_spec_links(const int32_t *nch, const gss_chain_t *chain, int nblk, int n_per_blk,
                   const gss_spec_in_t *in, const gss_spec_t *spec, gss_spec_link_t *link,
                   int threads);
int gss_carr_chain_linked(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                          const gss_chain_t *chain, int nblk, int n_per_blk,
                          const gss_spec_in_t *in, const gss_spec_t *spec,
                          const gss_spec_link_t *link, int threads, int *n_hit);
/* Move to run block `block` (>= the next block) without producing the blocks in between: only the
   30 s updates are replayed (nav frames, ephemeris steps, allocation), and the ranges of the
   block before the target (rho0 of computeCodePhase).  The slot carriers are unknown afterwards:
   gss_scn_next fails until gss_scn_set_carrier; gss_scn_next_deferred works.                */
int gss_scn_seek(gss_scn *s, int64_t block, int threads);
/* The planner's carrier per slot at the next block (get) / set it (after a seek).             */
int gss_scn_carrier(const gss_scn *s, double *carr);
int gss_scn_set_carrier(gss_scn *s, const double *carr);

/* Nav-word table rows produced so far ([n][GSS_NAV_WORDS]); valid until the next gss_scn_next. */
int gss_scn_nav_table(const gss_scn *s, const uint32_t **rows, int *n_rows);

/* Packed C/A codes for PRN 1..32 into out[32][GSS_CA_WORDS] (row prn-1).                      */
int gss_ca_table(uint32_t *out);

/* ---- the 30 s producers on the GPU ---------------------------------------------
   What the 30 s cadence produces for the sample loop -- the C/A chips (codegen, gpssim.c:132-171)
   and each channel's LNAV frame words with parity (generateNavMsg, gpssim.c:1467-1547) -- built
   on the device.  The host keeps what needs libm-exact doubles: ephemeris-to-subframe packing
   (eph2sbf, gpssim.c:490-665), allocation and ranges.  A nav-table row is described by its
   source: the frame's subframe data words, TOW count and week, and where its first ten words
   (the previous frame's subframe 5) come from.                                                */
#define GSS_NAV_HEAD_INIT   (-1)   /* rebuilt from sbf[4] with tow (a newly allocated channel) */
#define GSS_NAV_HEAD_GIVEN  (-2)   /* in head[] (the first row after a seek)                    */
typedef struct {
    uint32_t sbf[5][10];     /* subframe data words (no TOW/WN/parity) at the frame's update   */
    uint32_t tow;            /* g0.sec / 6: the TOW count before the first subframe            */
    uint32_t wn;             /* g0.week % 1024                                                  */
    int32_t  prev;           /* >= 0: row whose words 50..59 are this row's words 0..9, else
                                GSS_NAV_HEAD_INIT / GSS_NAV_HEAD_GIVEN                          */
    int32_t  next;           /* row continuing this one (its prev), or -1                       */
    uint32_t head[10];       /* words 0..9 for GSS_NAV_HEAD_GIVEN                               */
} gss_nav_src_t;             /* 256 bytes; row r of gss_scn_nav_table is built from source r   */

/* The sources of the rows of gss_scn_nav_table ([n], same order); next links within the table. */
int gss_scn_nav_sources(const gss_scn *s, const gss_nav_src_t **src, int *n_rows);
/* Rows [first, first + n) of a nav table from their sources src[0 .. n) (host: the producers'
   reference); rows before `first` must already be in rows (a source's prev may point there). */
int gss_nav_rows_host(const gss_nav_src_t *src, int first, int n, uint32_t *rows);
/* The same on the device (asynchronous on `stream`): src, rows are device pointers, src holds
   the sources of rows [first, first + n) at src[0 .. n); one lane per chain of rows.          */
int gss_nav_rows_device(gss_dev *d, const gss_nav_src_t *src, int first, int n, uint32_t *rows,
                        void *stream);
/* The packed C/A table of gss_ca_table built on the device into out[32][GSS_CA_WORDS].        */
int gss_ca_table_device(gss_dev *d, uint32_t *out, void *stream);

/* Wall time [s] the host planner spent so far (control plane + carrier chain).                */
double gss_scn_plan_seconds(const gss_scn *s);

int gss_scn_close(gss_scn *s);

/* ------------------------------------------------------------------------------------------ */
/* Streaming driver: the reference's block loop (gpssim.c:2154-2353) end to end               */
/* ------------------------------------------------------------------------------------------ */
/* Byte sink of gss_run: called in run order on the calling thread with the exact output bytes
   of `nblocks` consecutive blocks starting at run block `first_block` (what the reference
   fwrite()s for them).  Return 0 to continue, non-zero to stop the run (GSS_E_IO).            */
typedef int (*gss_sink_fn)(void *user, const void *bytes, size_t n, int64_t first_block,
                           int nblocks);

/* Run blocks [first_block, first_block + n_blocks) of scenario s (n_blocks < 0: to the end) on
   device d and stream their bytes to `sink`.  Planning (gss_scn_next on `threads` host
   threads, in its own thread), upload, both kernel stages, download into pinned buffers and the
   sink overlap; `batch` blocks per launch (capped at 256 MiB of output).  Blocks before
   first_block are planned (the carrier chain is serial) but not synthesised: a rank of a
   multi-GPU run passes its own range and writes at first_block * gss_block_bytes().           */
int gss_run(gss_dev *d, gss_scn *s, int64_t first_block, int64_t n_blocks, int batch,
            int threads, gss_sink_fn sink, void *user);

/* gss_run for one process of a multi-process run, planned once per node (no process plans another
   process's blocks): with carr_in set, the planner thread seeks to first_block (gss_scn_seek),
   produces the range's rows (gss_scn_next_deferred), calls carr_in for the 16 slot carriers at
   first_block (it may block until the process before has them), walks the carrier chain over
   the range (gss_carr_chain) and hands the end state to carr_out (if set) -- before the first
   batch renders.  Both callbacks return 0, or non-zero to abort the run (GSS_E_IO).
   opts == NULL: gss_run.  carr_in == NULL: blocks before first_block are planned and dropped
   as in gss_run; impair, jam and echo apply either way (fir needs carr_in == NULL).          */
typedef struct gss_run_opts {
    int (*carr_in)(void *user, double *carr);             /* [GSS_MAXCH], out                  */
    int (*carr_out)(void *user, const double *carr);      /* [GSS_MAXCH]                       */
    void *carr_user;
    /* Optional: the chain speculated across ranks.  Called twice (round 0: by the lines, round
       1: by an exact chain from the first prediction) before carr_in, with this range's map of
       the slot carriers, map[3 * GSS_MAXCH] = {start (the run's initial carriers when the range
       starts at block 0, else 0), add, reset}: the range takes x to reset ? add : (x + add) mod
       1 per slot.  It publishes the map to the ranks after this one and returns in start_out
       the composition of the maps of the ranks before it (gpssim_amd/shard.py compose_start).
       The walks then run before carr_in, and from carr_in to carr_out only the records' chain
       is left.  Exact whatever the predictions.  A rank that is given the
       callback but does not speculate (GSS_RUN_SPEC=0 or GSS_RUN_REC=0 in its environment, or
       no fast path) calls it once with round -1 and map == start_out == NULL, so that the
       ranks after it can fail at once instead of waiting for maps that never come.          */
    int (*carr_predict)(void *user, int round, const double *map, double *start_out);
    /* Optional (NULL: off): additive noise.  Every block renders at SC16 and the impairment
       (gss_impair_device, sample0 = run block * n_per_blk) writes the scenario's format.       */
    const gss_impair_t *impair;
    /* Optional (n_jam 0: none): jammers, copied when the run starts.  They need impair (its
       shift; sigma_q8 = 0 for no noise); gss_jam_device then takes gss_impair_device's place. */
    const gss_jam_t *jam;
    int n_jam;
    /* Optional (n_echo 0: none): multipath echoes, copied when the run starts.  They need impair
       too; gss_echo_device runs on each slot's SC16 render and rows before the impairment or
       the jammers.                                                                            */
    const gss_echo_t *echo;
    int n_echo;
    /* Optional (null: none): the front-end filter, copied when the run starts.  It needs impair
       too (sigma_q8 = 0: the plain chain) and no carr_in.  The impairment or the jammers then
       write SC16 in place and gss_fir_device writes the run's format; the run keeps the last
       n_taps - 1 unfiltered samples of each slot on the device as the next slot's halo, and with
       first_block > 0 it also renders the blocks that hold the n_taps - 1 samples before the
       range (one block) and keeps them from the sink, so the bytes do not depend on batches or
       on where a range starts.  The scenario must not have passed those blocks (GSS_E_STATE).
       A filtered run waits for a slot's GPU proof before it renders the slot.                 */
    const gss_fir_t *fir;
} gss_run_opts_t;
int gss_run_ex(gss_dev *d, gss_scn *s, int64_t first_block, int64_t n_blocks, int batch,
               int threads, gss_sink_fn sink, void *user, const gss_run_opts_t *opts);


/* Exact carrier-chain helpers (exported for tests): advance the reference recurrence
   carr += step; wrap into [0,1) (gpssim.c:2245-2250) by n samples, exactly.                   */
double gss_carr_advance(double carr, double step, int64_t n);
/* Same over one block of n samples, also recording the GSS_NCK carrier checkpoints of the
   block (ck[j] = phase at sample (j*n)/GSS_NCK) for gss_synth_*'s carr_ck.  Returns the phase
   after the block, i.e. the next block's carr0.                                               */
double gss_carr_advance_ck(double carr, double step, int n, double *ck);
/* Same for the code phase with its chip/bit/word counters (gpssim.c:2212-2241).               */
double gss_code_advance(double code, double step, int64_t n, int32_t *icode, int32_t *ibit,
                        int32_t *iword);

/* The 512-entry carrier tables the sample loop uses (gpssim.c:15-83), generated.             */
int gss_lut(int32_t *sin512, int32_t *cos512);

const char *gss_last_error(void);
const char *gss_version(void);
/* Build configuration of the kernels, e.g. "lin_mfma=1 lin_ch=16 arch=gfx950" (lin_mfma: the fast
   path accumulates f16 x f16 products in f32 on the matrix cores, exact integer sums; 0: int64
   multiply-adds on the VALU).                                                                 */
const char *gss_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* GPSSIM_AMD_H */
