/*
 * gss_obs.h — the observables of tracked signals as host/device functions, exact integer
 * arithmetic (include/gpssim_amd.h, gss_obs_t).  The same code runs in the GPU
 * kernel (csrc/hip/gss_obs.hip) and in the host statement gss_obs_host (csrc/host/obs.c);
 * tests/obs_oracle.py holds an independent restatement in Python integers.
 *
 * Every form walks the records, not the instants: record e with its prefixes phi_e and A_e owns
 * the instants k with s_e <= t_first + k step < s_e + n_e, the range [gss_obs_kbelow(s_e),
 * gss_obs_kbelow(s_e + n_e)), and writes them (gss_obs_emit); the instants before the first
 * record and from the end of the last one on are marked (gss_obs_mark).  The sums are taken
 * modulo 2^64 in uint64, so their order does not matter and nothing overflows.
 */
#ifndef GSS_OBS_H
#define GSS_OBS_H

#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_trk.h"

#define GSS_OBS_TMAX   (1LL << 62)             /* the last instant                              */
#define GSS_OBS_KMAX   (1 << 30)               /* instants per job                              */
#define GSS_OBS_T0MAX  (1LL << 61)             /* |t_first|                                     */

/* 0, or -1 for instants the calls reject */
GSS_ACQ_HD int gss_obs_check(int64_t t_first, int64_t step, int32_t n_fix)
{
    if (n_fix < 0 || n_fix > GSS_OBS_KMAX || step < 1 || t_first > GSS_OBS_T0MAX || t_first < -GSS_OBS_T0MAX)
        return -1;
    if (n_fix > 1 && step > (GSS_OBS_TMAX - t_first) / (n_fix - 1))
        return -1;
    return 0;
}

/* how many instants k < n_fix lie below sample s: t_first + k step < s */
GSS_ACQ_HD int32_t gss_obs_kbelow(int64_t s, int64_t t_first, int64_t step, int32_t n_fix)
{
    if (s <= t_first)
        return 0;
    const uint64_t a = (uint64_t)s - (uint64_t)t_first;      /* > 0; the difference fits uint64 */
    const uint64_t q = (a - 1) / (uint64_t)step + 1;
    return q < (uint64_t)n_fix ? (int32_t)q : n_fix;
}

/* what a record (first sample s, carrier step w, code step cs_nom + dcs) adds to the prefixes
   when the next record starts at s_next */
GSS_ACQ_HD void gss_obs_delta(int64_t s, int32_t w, int32_t dcs, int64_t s_next, int64_t cs_nom,
                              uint64_t *dphi, uint64_t *dA)
{
    const uint64_t n = (uint64_t)s_next - (uint64_t)s;
    *dphi = n * (uint64_t)(cs_nom + dcs) - (uint64_t)GSS_TRK_M;
    *dA = n * (uint64_t)(int64_t)w;
}

/* the last record's length: tracking's, or 0 for a state tracking never leaves */
GSS_ACQ_HD int64_t gss_obs_last_len(uint64_t phi, int64_t cs)
{
    if (cs <= 0 || phi >= (uint64_t)GSS_TRK_M)
        return 0;
    return (int64_t)(((uint64_t)GSS_TRK_M - phi + (uint64_t)cs - 1) / (uint64_t)cs);
}

/* record e (s, w, dcs) with prefixes phi and A owns the instants [ka, kb) of its job's row obs */
GSS_ACQ_HD void gss_obs_emit(int64_t s, int32_t w, int32_t dcs, int32_t e, uint64_t phi,
                             uint64_t A, int64_t cs_nom, int64_t t_first, int64_t step,
                             int32_t ka, int32_t kb, gss_obs_t *obs)
{
    const uint64_t cs = (uint64_t)(cs_nom + dcs), ws = (uint64_t)(int64_t)w;
    for (int32_t k = ka; k < kb; k++) {
        const uint64_t dt = (uint64_t)(t_first + (int64_t)k * step) - (uint64_t)s;
        gss_obs_t o;
        o.code = (int64_t)(phi + dt * cs);
        o.adr = (int64_t)(A + dt * ws);
        o.epoch = e;
        o.w = w;
        o.pad = 0;
        obs[k] = o;
    }
}

/* instants [ka, kb) lie outside the job's records */
GSS_ACQ_HD void gss_obs_mark(int32_t ka, int32_t kb, int32_t stride, gss_obs_t *obs)
{
    gss_obs_t o;
    o.code = 0;
    o.adr = 0;
    o.epoch = -1;
    o.w = 0;
    o.pad = 0;
    for (int32_t k = ka; k < kb; k += stride)
        obs[k] = o;
}

/* one job from its first record to its last, serially: the host's statement and the kernel's
   plain form */
GSS_ACQ_HD void gss_obs_walk(const gss_trk_rec_t *rec, int32_t count, int64_t cs_nom,
                             int64_t t_first, int64_t step, int32_t n_fix, gss_obs_t *obs)
{
    if (count < 1) {
        gss_obs_mark(0, n_fix, 1, obs);
        return;
    }
    uint64_t phi = 0, A = 0;
    int32_t ka = gss_obs_kbelow(rec[0].s, t_first, step, n_fix);
    gss_obs_mark(0, ka, 1, obs);
    for (int32_t e = 0; e < count; e++) {
        const int64_t s = rec[e].s;
        const int32_t w = rec[e].w, dcs = rec[e].dcs;
        uint64_t dphi = 0, dA = 0;
        int64_t end;
        if (e + 1 < count) {
            end = rec[e + 1].s;
            gss_obs_delta(s, w, dcs, end, cs_nom, &dphi, &dA);
        } else {
            end = s + gss_obs_last_len(phi, cs_nom + dcs);
        }
        const int32_t kb = gss_obs_kbelow(end, t_first, step, n_fix);
        gss_obs_emit(s, w, dcs, e, phi, A, cs_nom, t_first, step, ka, kb, obs);
        ka = kb;
        phi += dphi;
        A += dA;
    }
    gss_obs_mark(ka, n_fix, 1, obs);
}

#endif /* GSS_OBS_H */
