/*
 * track.c — signal tracking on the host: the plain-C statement of csrc/common/gss_trk.h
 * (gss_track_host), the default loop gains (gss_trk_defaults) and the job that continues an
 * acquisition peak (gss_trk_job_from_peak).  The reference has no receiver; this is an extension
 * that measures its samples.  gss_track_host is what the GPU kernel (csrc/hip/gss_track.hip) is
 * tested against.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_trk.h"

/* the argument checks every tracking call shares */
int gss_trk_check_args(const gss_trk_cfg_t *cfg, int64_t N, const gss_trk_job_t *jobs, int n_job,
                       int64_t pitch)
{
    const char *why;
    if (!cfg || !jobs || N < 0 || n_job < 1 || pitch < 0 || pitch > 0x7FFFFFFF)
        return gss_fail(GSS_E_ARG, "invalid tracking arguments");
    if (gss_trk_check(cfg, &why) != 0)
        return gss_fail(GSS_E_ARG, "invalid tracking configuration: %s", why);
    for (int j = 0; j < n_job; j++) {
        if (jobs[j].prn < 1 || jobs[j].prn > 32)
            return gss_fail(GSS_E_ARG, "tracking job %d: PRN %d outside 1..32", j, jobs[j].prn);
        /* s0 + an epoch + the samples the kernel loads ahead must not leave int64 */
        if (jobs[j].s0 < 0 || jobs[j].s0 > GSS_TRK_S0MAX || jobs[j].n_epoch < 0 ||
            jobs[j].n_epoch > pitch)
            return gss_fail(GSS_E_ARG,
                            "tracking job %d: s0 outside 0..2^62 or n_epoch outside 0..pitch", j);
    }
    return 0;
}

int gss_trk_defaults(int32_t fs_hz, int32_t fmt, gss_trk_cfg_t *cfg)
{
    const char *why;
    if (!cfg || fs_hz < 1)
        return gss_fail(GSS_E_ARG, "invalid tracking arguments");
    const double T = 1e-3, wn = 34.0, two_pi_fs = 2.0 * 3.14159265358979323846 * fs_hz;
    const double p34 = 17179869184.0;
    cfg->fs_hz = fs_hz;
    cfg->fmt = fmt;
    cfg->n_pull = 300;
    cfg->Ki = (int32_t)floor(wn * wn * T * p34 / two_pi_fs + 0.5);
    cfg->Kp = (int32_t)floor(1.414 * wn * p34 / two_pi_fs + 0.5);
    cfg->Kf = (int32_t)floor(0.05 * p34 / (two_pi_fs * T) + 0.5);
    cfg->Kd = (int32_t)floor(8.0 * 8589934592.0 / fs_hz + 0.5);
    if (gss_trk_check(cfg, &why) != 0)
        return gss_fail(GSS_E_ARG, "invalid tracking configuration: %s", why);
    return 0;
}

int gss_trk_job_from_peak(const gss_acq_t *a, const gss_acq_peak_t *peak, int64_t sample0,
                          int32_t n_epoch, gss_trk_job_t *job)
{
    if (!a || !peak || !job || a->fs_hz < 1000 || a->bin_hz < 1 || sample0 < 0 || peak->tau < 0 ||
        peak->prn < 1 || peak->prn > 32 || n_epoch < 0)
        return gss_fail(GSS_E_ARG, "invalid tracking-job arguments");
    job->s0 = sample0 + peak->tau;
    job->prn = peak->prn;
    job->w0 = (int32_t)gss_acq_step(peak->bin, a->bin_hz, a->fs_hz);
    job->n_epoch = n_epoch;
    job->pad = 0;
    return 0;
}

typedef struct {
    const gss_trk_cfg_t *cfg;
    const void *samples;
    int64_t N, pitch, cs_nom;
    const gss_trk_job_t *jobs;
    gss_trk_rec_t *rec;
    int32_t *count;
    int32_t lut_c[512], lut_s[512];
    uint32_t ca[32 * GSS_CA_WORDS];
} trk_run;

static void track_part(void *arg, int part)
{
    const trk_run *r = (const trk_run *)arg;
    const gss_trk_job_t *job = &r->jobs[part];
    const uint32_t *ca = r->ca + (size_t)(job->prn - 1) * GSS_CA_WORDS;
    gss_trk_rec_t *rec = r->rec + (size_t)part * r->pitch;
    const int fmt = r->cfg->fmt;
    gss_trk_state_t t;
    gss_trk_init(&t, job, r->cs_nom);
    while (t.e < job->n_epoch) {
        const int32_t n = gss_trk_len(t.phi, t.cs);
        if (t.s + n > r->N)
            break;
        int64_t q[6] = {0, 0, 0, 0, 0, 0};
        int64_t c = t.phi;
        uint32_t th = t.th;
        for (int32_t i = 0; i < n; i++, c += t.cs, th += (uint32_t)t.w) {
            int32_t xi, xq;
            gss_acq_sample(r->samples, fmt, t.s + i, &xi, &xq);
            const int32_t co = r->lut_c[th >> 23], si = r->lut_s[th >> 23];
            const int64_t yi = xi * co + xq * si, yq = xq * co - xi * si;
            const int32_t e = gss_acq_replica(ca, gss_trk_chip_early(c));
            const int32_t p = gss_acq_replica(ca, (int32_t)(c >> 32));
            const int32_t l = gss_acq_replica(ca, gss_trk_chip_late(c));
            q[0] += yi * e; q[1] += yq * e;
            q[2] += yi * p; q[3] += yq * p;
            q[4] += yi * l; q[5] += yq * l;
        }
        gss_trk_update(&t, r->cfg, r->cs_nom, q, n, &rec[t.e]);
    }
    r->count[part] = t.e;
}

int gss_track_host(const gss_trk_cfg_t *cfg, const void *samples, int64_t N,
                   const gss_trk_job_t *jobs, int n_job, gss_trk_rec_t *rec, int64_t pitch,
                   int32_t *count, int threads)
{
    int rc = gss_trk_check_args(cfg, N, jobs, n_job, pitch);
    if (rc)
        return rc;
    if (!samples || !rec || !count || (cfg->fmt == GSS_FMT_SC16 && ((uintptr_t)samples & 1)))
        return gss_fail(GSS_E_ARG, "invalid tracking buffers");
    trk_run *r = (trk_run *)calloc(1, sizeof *r);
    if (!r)
        return gss_fail(GSS_E_NOMEM, "out of memory");
    r->cfg = cfg;
    r->samples = samples;
    r->N = N;
    r->pitch = pitch;
    r->cs_nom = gss_trk_cs_nom(cfg->fs_hz);
    r->jobs = jobs;
    r->rec = rec;
    r->count = count;
    gss_lut(r->lut_s, r->lut_c);
    gss_ca_table(r->ca);
    rc = gss_pool_run(threads < 1 ? 1 : threads, n_job, track_part, r);
    free(r);
    return rc;
}
