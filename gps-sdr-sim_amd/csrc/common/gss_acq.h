/*
 * gss_acq.h — the acquisition search as host/device functions, exact integer arithmetic
 * (include/gpssim_amd.h, gss_acq_t).  The same code runs in the GPU kernels
 * (csrc/hip/gss_acquire.hip) and in the host statement gss_acquire_host (csrc/host/acquire.c);
 * tests/acq_oracle.py holds an independent numpy restatement.
 *
 *   sample   SC16 / SC08: the int16 / int8 pair; SC01: bit set -> +1, clear -> -1, component c
 *            = 2 n (I), 2 n + 1 (Q) at bit 7 - c % 8 of byte c / 8 (gpssim.c:2268-2274)
 *   wipe     idx = ((n step) mod 2^32) >> 23 into the 512-entry tables; yI = xI c + xQ s,
 *            yQ = xQ c - xI s (|y| <= 2 * 32768 * 250 < 2^24)
 *   quantise q = clamp((y + ((1 << sh) >> 1)) >> sh, -127, 127)
 *   replica  chip (i 1023000 / fs) mod 1023 of the packed C/A row: set -> +1, clear -> -1
 */
#ifndef GSS_ACQ_H
#define GSS_ACQ_H

#include <stdint.h>
#include "gpssim_amd.h"

#if defined(__HIPCC__)
#define GSS_ACQ_HD __host__ __device__ inline
#else
#define GSS_ACQ_HD static inline
#endif

#define GSS_ACQ_LMAX (1 << 20)           /* samples per coherent window                        */
#define GSS_ACQ_MMAX 1000                /* windows                                            */

typedef struct gss_acq_dims {
    int32_t L, T, E, n_prn, n_bin;
    int64_t N;
    int32_t prn[32];                     /* the selected PRNs, ascending                       */
} gss_acq_dims_t;

/* the derived sizes; 0, or -1 with *why set for a search the calls reject */
GSS_ACQ_HD int gss_acq_dims(const gss_acq_t *a, gss_acq_dims_t *d, const char **why)
{
    *why = "";
    if (a->fs_hz < 1000) { *why = "fs_hz below 1000"; return -1; }
    if (a->fmt != GSS_FMT_SC16 && a->fmt != GSS_FMT_SC08 && a->fmt != GSS_FMT_SC01) {
        *why = "fmt is not 16, 8 or 1"; return -1;
    }
    if (a->coh_ms < 1) { *why = "coh_ms below 1"; return -1; }
    if (a->n_coh < 1 || a->n_coh > GSS_ACQ_MMAX) { *why = "n_coh outside 1..1000"; return -1; }
    if (a->bin_hz < 1) { *why = "bin_hz below 1"; return -1; }
    if (a->n_half < 0 || a->n_half > 16384 || (int64_t)a->n_half * a->bin_hz >= ((int64_t)1 << 30)) {
        *why = "n_half outside 0..16384 or n_half * bin_hz >= 2^30"; return -1;
    }
    if (a->qshift < -1 || a->qshift > 24) { *why = "qshift outside -1..24"; return -1; }
    if (a->prn_mask == 0) { *why = "empty prn_mask"; return -1; }
    const int64_t L = (int64_t)a->fs_hz * a->coh_ms / 1000;
    if (L > GSS_ACQ_LMAX) { *why = "coherent window above 2^20 samples"; return -1; }
    d->L = (int32_t)L;
    d->T = (int32_t)(((int64_t)a->fs_hz + 999) / 1000);
    d->E = (int32_t)((2 * (int64_t)a->fs_hz + 1022999) / 1023000) + 1;
    if (d->T <= 2 * d->E + 1) { *why = "code period no longer than the excluded zone"; return -1; }
    d->N = (int64_t)a->n_coh * L + d->T - 1;
    d->n_bin = 2 * a->n_half + 1;
    d->n_prn = 0;
    for (int p = 0; p < 32; p++) {
        d->prn[p] = 0;
        if (a->prn_mask >> p & 1)
            d->prn[d->n_prn++] = p + 1;
    }
    return 0;
}

/* carrier step of bin k: floor((f_k 2^32 + fs / 2) / fs) mod 2^32 */
GSS_ACQ_HD uint32_t gss_acq_step(int32_t k, int32_t bin_hz, int32_t fs)
{
    const int64_t num = (int64_t)k * bin_hz * 4294967296LL + fs / 2;
    int64_t q = num / fs;
    if (num % fs < 0)
        q--;
    return (uint32_t)q;
}

GSS_ACQ_HD void gss_acq_sample(const void *s, int fmt, int64_t n, int32_t *xi, int32_t *xq)
{
    if (fmt == GSS_FMT_SC16) {
        *xi = ((const int16_t *)s)[2 * n];
        *xq = ((const int16_t *)s)[2 * n + 1];
    } else if (fmt == GSS_FMT_SC08) {
        *xi = ((const int8_t *)s)[2 * n];
        *xq = ((const int8_t *)s)[2 * n + 1];
    } else {
        const uint32_t b = ((const uint8_t *)s)[n >> 2];
        const int sh = 7 - 2 * (int)(n & 3);
        *xi = (b >> sh & 1) ? 1 : -1;
        *xq = (b >> (sh - 1) & 1) ? 1 : -1;
    }
}

/* the bytes that hold n samples (SC01: whole bytes, four samples each) */
GSS_ACQ_HD size_t gss_acq_bytes(int fmt, int64_t n)
{
    return fmt == GSS_FMT_SC16 ? (size_t)n * 4 : fmt == GSS_FMT_SC08 ? (size_t)n * 2
                                                                     : (size_t)(n + 3) / 4;
}

/* the automatic shift from the input's component maxima */
GSS_ACQ_HD int32_t gss_acq_auto_shift(int32_t max_i, int32_t max_q)
{
    const int32_t v = 250 * (max_i + max_q);
    int32_t sh = 0;
    while ((v >> sh) > 127)
        sh++;
    return sh;
}

GSS_ACQ_HD int32_t gss_acq_quant(int32_t y, int32_t sh)
{
    const int32_t v = (y + ((1 << sh) >> 1)) >> sh;
    return v < -127 ? -127 : v > 127 ? 127 : v;
}

/* a sample wiped by (c, s) = gss_lut's (cos, sin) at gss_acq_lut_idx, and quantised */
GSS_ACQ_HD void gss_acq_wipe(int32_t xi, int32_t xq, int32_t c, int32_t s, int32_t sh,
                             int32_t *qi, int32_t *qq)
{
    *qi = gss_acq_quant(xi * c + xq * s, sh);
    *qq = gss_acq_quant(xq * c - xi * s, sh);
}

GSS_ACQ_HD uint32_t gss_acq_lut_idx(int64_t n, uint32_t step)
{
    return ((uint32_t)n * step) >> 23;
}

/* replica sample i of PRN row `ca` (GSS_CA_WORDS packed words): +1 / -1 */
GSS_ACQ_HD int32_t gss_acq_chip_idx(int64_t i, int32_t fs)
{
    return (int32_t)((uint64_t)i * 1023000u / (uint32_t)fs % 1023u);
}

GSS_ACQ_HD int32_t gss_acq_replica(const uint32_t *ca, int32_t chip)
{
    return (ca[chip >> 5] >> (chip & 31) & 1) ? 1 : -1;
}

/* is cell t outside the zone excluded around peak tau (circular in T)? */
GSS_ACQ_HD int gss_acq_floor_cell(int32_t t, int32_t tau, int32_t T, int32_t E)
{
    int32_t d = t > tau ? t - tau : tau - t;
    if (T - d < d)
        d = T - d;
    return d > E;
}

#endif /* GSS_ACQ_H */
