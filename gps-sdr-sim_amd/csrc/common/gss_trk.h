/*
 * gss_trk.h — the tracking loops as host/device functions, exact integer arithmetic
 * (include/gpssim_amd.h, gss_trk_cfg_t).  The same code runs in the GPU kernel
 * (csrc/hip/gss_track.hip) and in the host statement gss_track_host (csrc/host/track.c);
 * tests/trk_oracle.py holds an independent numpy restatement.  A caller sums the six correlator
 * outputs of an epoch in any order (int64 sums do not depend on it) and hands them to
 * gss_trk_update, which is the whole feedback path.
 */
#ifndef GSS_TRK_H
#define GSS_TRK_H

#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_acq.h"

#define GSS_TRK_M      (1023LL << 32)          /* one code period in 2^-32 chip                 */
#define GSS_TRK_HALF   (1LL << 31)             /* the early / late offset: half a chip          */
#define GSS_TRK_KMAX   (1 << 30)               /* the gains' upper limit                        */
#define GSS_TRK_WSPAN  (2147483648LL / 1540 + 2)   /* |w / 1540| stays below this               */
#define GSS_TRK_CSMIN  (GSS_TRK_M >> 23)       /* the code step stays above this: n < 2^23      */
#define GSS_TRK_S0MAX  (1LL << 62)             /* a job's first sample: s + n stays in int64    */

typedef struct gss_trk_state {
    int64_t  s;                  /* next epoch's first sample                                   */
    int64_t  phi;                /* code phase there                                            */
    int64_t  W;                  /* carrier accumulator, 16 more fraction bits than w           */
    int64_t  cs;                 /* code step                                                   */
    uint32_t th;                 /* carrier phase                                               */
    int32_t  w;                  /* carrier step                                                */
    int32_t  up, vp;             /* (u, v) of the epoch before                                  */
    int32_t  e;                  /* epochs done                                                 */
    int32_t  done;               /* the job ran out of samples                                  */
    int32_t  n_hint, pad;        /* the last epoch's length (0: none yet)                       */
} gss_trk_state_t;               /* 64 bytes                                                    */

GSS_ACQ_HD int64_t gss_trk_cs_nom(int32_t fs)
{
    return (1023000LL * 4294967296LL + fs / 2) / fs;
}

/* 0, or -1 with *why set for a configuration the calls reject */
GSS_ACQ_HD int gss_trk_check(const gss_trk_cfg_t *c, const char **why)
{
    *why = "";
    if (c->fs_hz < 1000) { *why = "fs_hz below 1000"; return -1; }
    if (c->fmt != GSS_FMT_SC16 && c->fmt != GSS_FMT_SC08 && c->fmt != GSS_FMT_SC01) {
        *why = "fmt is not 16, 8 or 1"; return -1;
    }
    if (c->n_pull < 0) { *why = "n_pull below 0"; return -1; }
    if (c->Kf < 0 || c->Kf > GSS_TRK_KMAX || c->Ki < 0 || c->Ki > GSS_TRK_KMAX ||
        c->Kp < 0 || c->Kp > GSS_TRK_KMAX || c->Kd < 0 || c->Kd > GSS_TRK_KMAX) {
        *why = "a gain outside 0..2^30"; return -1;
    }
    /* |w / 1540| < WSPAN for every int32 w, |(Kd D_dll) >> 16| <= Kd / 4 + 1 as |D_dll| <= 2^14;
       a code step above M / 2^23 keeps every epoch shorter than 2^23 samples */
    const int64_t span = GSS_TRK_WSPAN + c->Kd / 4 + 2, cn = gss_trk_cs_nom(c->fs_hz);
    if (cn - span <= GSS_TRK_CSMIN || cn + span >= GSS_TRK_M) {
        *why = "the code step could reach M / 2^23 or a whole code period"; return -1;
    }
    return 0;
}

/* samples of the epoch that starts at code phase phi: ceil((M - phi) / cs), below 2^23 for every
   code step gss_trk_check admits */
GSS_ACQ_HD int32_t gss_trk_len(int64_t phi, int64_t cs)
{
    return (int32_t)((GSS_TRK_M - phi + cs - 1) / cs);
}

/* the same without the division when the length is within one of `hint` */
GSS_ACQ_HD int32_t gss_trk_len_hint(int64_t phi, int64_t cs, int32_t hint)
{
    const int64_t r = GSS_TRK_M - phi;
    for (int32_t n = hint - 1; hint > 1 && n <= hint + 1; n++)
        if ((int64_t)n * cs >= r && (int64_t)(n - 1) * cs < r)
            return n;
    return gss_trk_len(phi, cs);
}

/* chip indices of code phase c in [0, M) */
GSS_ACQ_HD int32_t gss_trk_chip_early(int64_t c)
{
    const int64_t x = c + GSS_TRK_HALF;
    return (int32_t)((x >= GSS_TRK_M ? x - GSS_TRK_M : x) >> 32);
}

GSS_ACQ_HD int32_t gss_trk_chip_late(int64_t c)
{
    const int64_t x = c - GSS_TRK_HALF;
    return (int32_t)((x < 0 ? x + GSS_TRK_M : x) >> 32);
}

GSS_ACQ_HD int64_t gss_trk_abs(int64_t a) { return a < 0 ? -a : a; }

GSS_ACQ_HD int64_t gss_trk_amb(int64_t a, int64_t b)
{
    a = gss_trk_abs(a);
    b = gss_trk_abs(b);
    return a > b ? a + (b >> 1) : b + (a >> 1);
}

/* a / b, truncating, for b > 0 and a quotient below 2^31 in size.  On the device the 64-bit
   division is a long instruction sequence on the epoch's critical path: there a double estimate
   (off by at most one: three roundings of 2^-53 on a quotient below 2^31) is corrected with the
   exact remainder, which gives the same value. */
GSS_ACQ_HD int64_t gss_trk_quot(int64_t a, int64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t aa = a < 0 ? -a : a;
    int64_t q = (int64_t)((double)aa / (double)b);
    int64_t r = aa - q * b;
    while (r < 0) {
        q--;
        r += b;
    }
    while (r >= b) {
        q++;
        r -= b;
    }
    return a < 0 ? -q : q;
#else
    return a / b;
#endif
}

GSS_ACQ_HD void gss_trk_init(gss_trk_state_t *t, const gss_trk_job_t *j, int64_t cs_nom)
{
    t->s = j->s0;
    t->phi = 0;
    t->W = (int64_t)j->w0 * 65536;
    t->cs = cs_nom + j->w0 / 1540;
    t->th = 0;
    t->w = j->w0;
    t->up = t->vp = 0;
    t->e = 0;
    t->done = 0;
    t->n_hint = 0;
    t->pad = 0;
}

/* the epoch of n samples with sums q[6] = IE QE IP QP IL QL is over: its record, and the state
   of the next epoch */
GSS_ACQ_HD void gss_trk_update(gss_trk_state_t *t, const gss_trk_cfg_t *c, int64_t cs_nom,
                               const int64_t *q, int32_t n, gss_trk_rec_t *r)
{
    r->IE = q[0]; r->QE = q[1]; r->IP = q[2]; r->QP = q[3]; r->IL = q[4]; r->QL = q[5];
    r->s = t->s;
    r->w = t->w;
    r->dcs = (int32_t)(t->cs - cs_nom);

    const int64_t m = gss_trk_amb(q[2], q[3]);
    const int32_t u = m ? (int32_t)gss_trk_quot(q[2] * 16384, m) : 0;
    const int32_t v = m ? (int32_t)gss_trk_quot(q[3] * 16384, m) : 0;
    const int64_t d_pll = u < 0 ? -v : v;
    int64_t d_fll = 0;
    if (t->e > 0) {
        const int64_t cross = (int64_t)t->up * v - (int64_t)t->vp * u;
        const int64_t dot = (int64_t)t->up * u + (int64_t)t->vp * v;
        d_fll = (dot < 0 ? -cross : cross) >> 14;
    }
    const int64_t me = gss_trk_amb(q[0], q[1]), ml = gss_trk_amb(q[4], q[5]);
    const int64_t d_dll = me + ml ? gss_trk_quot((me - ml) * 16384, me + ml) : 0;

    t->th += (uint32_t)n * (uint32_t)t->w;
    t->phi += (int64_t)n * t->cs - GSS_TRK_M;
    t->s += n;
    if (t->e < c->n_pull) {
        t->W = (int64_t)((uint64_t)t->W + (uint64_t)(c->Kf * d_fll));
        t->w = (int32_t)(uint32_t)(uint64_t)(t->W >> 16);
    } else {
        t->W = (int64_t)((uint64_t)t->W + (uint64_t)(c->Ki * d_pll));
        t->w = (int32_t)(uint32_t)(((uint64_t)t->W + (uint64_t)(c->Kp * d_pll)) >> 16);
    }
    t->cs = cs_nom + t->w / 1540 + ((c->Kd * d_dll) >> 16);
    t->up = u;
    t->vp = v;
    t->e++;
    t->n_hint = n;
}

#endif /* GSS_TRK_H */
