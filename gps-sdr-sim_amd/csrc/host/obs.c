/*
 * obs.c — the observables of tracked signals on the host: the plain-C statement of
 * csrc/common/gss_obs.h (gss_obs_host).  It is what the GPU kernel (csrc/hip/gss_obs.hip) is
 * tested against, and what a caller whose records are in host memory uses.
 */
#include <stdlib.h>
#include "gss_host.h"
#include "../common/gss_obs.h"

/* the argument checks every observables call shares */
int gss_obs_check_args(int32_t fs_hz, int64_t pitch, int n_job, int64_t t_first, int64_t step,
                       int32_t n_fix)
{
    if (fs_hz < 1000 || pitch < 0 || pitch > 0x7FFFFFFF || n_job < 1)
        return gss_fail(GSS_E_ARG, "invalid observables arguments");
    if (gss_obs_check(t_first, step, n_fix) != 0)
        return gss_fail(GSS_E_ARG, "observables: n_fix outside 0..2^30, step below 1, |t_first| above "
                                   "2^61 or the last instant above 2^62");
    return 0;
}

typedef struct {
    const gss_trk_rec_t *rec;
    const int32_t *count;
    gss_obs_t *obs;
    int64_t pitch, cs_nom, t_first, step;
    int32_t n_fix;
} obs_run;

static void obs_part(void *arg, int part)
{
    const obs_run *r = (const obs_run *)arg;
    const gss_trk_rec_t *rec = r->rec + (size_t)part * r->pitch;
    gss_obs_walk(rec, r->count[part], r->cs_nom, r->t_first, r->step, r->n_fix,
                 r->obs + (size_t)part * r->n_fix);
}

int gss_obs_host(int32_t fs_hz, const gss_trk_rec_t *rec, int64_t pitch, const int32_t *count,
                 int n_job, int64_t t_first, int64_t step, int32_t n_fix, gss_obs_t *obs,
                 int threads)
{
    int rc = gss_obs_check_args(fs_hz, pitch, n_job, t_first, step, n_fix);
    if (rc)
        return rc;
    if (!count || (n_fix > 0 && !obs))
        return gss_fail(GSS_E_ARG, "invalid observables buffers");
    for (int j = 0; j < n_job; j++)
        if (count[j] < 0 || count[j] > pitch || (count[j] > 0 && !rec))
            return gss_fail(GSS_E_ARG, "observables job %d: count outside 0..pitch", j);
    obs_run r = {rec, count, obs, pitch, gss_trk_cs_nom(fs_hz), t_first, step, n_fix};
    return gss_pool_run(threads < 1 ? 1 : threads, n_job, obs_part, &r);
}
