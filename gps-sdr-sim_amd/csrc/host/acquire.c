/*
 * acquire.c — the acquisition search on the host: the plain-C statement of
 * csrc/common/gss_acq.h (gss_acquire_host), the truth labels of a channel row (gss_acq_expect)
 * and the detection threshold (gss_acq_threshold).  The reference has no receiver; this is an
 * extension that measures its samples.  gss_acquire_host is what the GPU kernels
 * (csrc/hip/gss_acquire.hip) are tested against.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_acq.h"

/* the argument checks every acquisition call shares: the sizes, or GSS_E_ARG */
int gss_acq_check(const gss_acq_t *a, gss_acq_dims_t *d)
{
    const char *why;
    if (!a)
        return gss_fail(GSS_E_ARG, "invalid acquisition arguments");
    if (gss_acq_dims(a, d, &why) != 0)
        return gss_fail(GSS_E_ARG, "invalid acquisition search: %s", why);
    if ((int64_t)a->bin_hz * a->coh_ms > 500)          /* not an error: the message alone */
        (void)gss_fail(0, "warning: bin_hz * coh_ms = %lld > 500 leaves Doppler holes",
                       (long long)a->bin_hz * a->coh_ms);
    return 0;
}

int gss_acq_sizes(const gss_acq_t *a, int32_t *L, int32_t *T, int64_t *N, int32_t *E,
                  int32_t *n_prn)
{
    gss_acq_dims_t d;
    const int rc = gss_acq_check(a, &d);
    if (rc)
        return rc;
    if (L) *L = d.L;
    if (T) *T = d.T;
    if (N) *N = d.N;
    if (E) *E = d.E;
    if (n_prn) *n_prn = d.n_prn;
    return 0;
}

typedef struct {
    const gss_acq_t *a;
    const gss_acq_dims_t *d;
    const void *samples;
    int32_t sh;
    int32_t lut_c[512], lut_s[512];
    int8_t *planes;              /* [n_bin][2][N]                                               */
    int8_t *rep;                 /* [n_prn][M L]                                                */
    uint64_t *grid;              /* [n_prn][n_bin][T]                                           */
    gss_acq_peak_t *peaks;
} acq_job;

static void wipe_part(void *arg, int part)
{
    acq_job *j = (acq_job *)arg;
    const gss_acq_t *a = j->a;
    const int64_t N = j->d->N;
    const uint32_t step = gss_acq_step(part - a->n_half, a->bin_hz, a->fs_hz);
    int8_t *qi = j->planes + (size_t)part * 2 * N, *qq = qi + N;
    for (int64_t n = 0; n < N; n++) {
        int32_t xi, xq, vi, vq;
        gss_acq_sample(j->samples, a->fmt, n, &xi, &xq);
        const uint32_t idx = gss_acq_lut_idx(n, step);
        gss_acq_wipe(xi, xq, j->lut_c[idx], j->lut_s[idx], j->sh, &vi, &vq);
        qi[n] = (int8_t)vi;
        qq[n] = (int8_t)vq;
    }
}

/* S_I, S_Q of one window: the plain sums (the compiler vectorises them) */
__attribute__((optimize("O3"))) static void
corr_window(const int8_t *qi, const int8_t *qq, const int8_t *r, int32_t L, int32_t *si,
            int32_t *sq)
{
    int32_t a = 0, b = 0;
    for (int32_t i = 0; i < L; i++) {
        a += (int32_t)qi[i] * r[i];
        b += (int32_t)qq[i] * r[i];
    }
    *si = a;
    *sq = b;
}

static void corr_part(void *arg, int part)                  /* part = bin * n_prn + prn slot */
{
    acq_job *j = (acq_job *)arg;
    const gss_acq_dims_t *d = j->d;
    const int M = j->a->n_coh;
    const int k = part / d->n_prn, p = part % d->n_prn;
    const int8_t *qi = j->planes + (size_t)k * 2 * d->N, *qq = qi + d->N;
    const int8_t *r = j->rep + (size_t)p * M * d->L;
    uint64_t *row = j->grid + ((size_t)p * d->n_bin + k) * d->T;
    for (int32_t tau = 0; tau < d->T; tau++) {
        uint64_t P = 0;
        for (int m = 0; m < M; m++) {
            int32_t si, sq;
            const size_t o = (size_t)m * d->L;
            corr_window(qi + tau + o, qq + tau + o, r + o, d->L, &si, &sq);
            P += (uint64_t)((int64_t)si * si) + (uint64_t)((int64_t)sq * sq);
        }
        row[tau] = P;
    }
}

static void peak_part(void *arg, int p)
{
    acq_job *j = (acq_job *)arg;
    const gss_acq_dims_t *d = j->d;
    const uint64_t *g = j->grid + (size_t)p * d->n_bin * d->T;
    gss_acq_peak_t *o = &j->peaks[p];
    size_t best = 0;
    for (size_t c = 1; c < (size_t)d->n_bin * d->T; c++)    /* ties: lowest k, then lowest tau */
        if (g[c] > g[best])
            best = c;
    const int32_t kb = (int32_t)(best / d->T), tau = (int32_t)(best % d->T);
    o->peak = g[best];
    o->tau = tau;
    o->bin = kb - j->a->n_half;
    o->prn = d->prn[p];
    o->floor_sum = 0;
    o->floor_cnt = 0;
    for (int32_t t = 0; t < d->T; t++)
        if (gss_acq_floor_cell(t, tau, d->T, d->E)) {
            o->floor_sum += g[(size_t)kb * d->T + t];
            o->floor_cnt++;
        }
}

int gss_acquire_host(const gss_acq_t *a, const void *samples, gss_acq_peak_t *peaks,
                     uint64_t *grid, int *qshift_out, int threads)
{
    gss_acq_dims_t d;
    int rc = gss_acq_check(a, &d);
    if (rc)
        return rc;
    if (!samples || !peaks || (a->fmt == GSS_FMT_SC16 && ((uintptr_t)samples & 1)))
        return gss_fail(GSS_E_ARG, "invalid acquisition buffers");
    if (threads < 1)
        threads = 1;
    acq_job *j = (acq_job *)calloc(1, sizeof *j);
    if (!j)
        return gss_fail(GSS_E_NOMEM, "out of memory");
    const size_t ML = (size_t)a->n_coh * d.L, cells = (size_t)d.n_prn * d.n_bin * d.T;
    j->a = a;
    j->d = &d;
    j->samples = samples;
    j->peaks = peaks;
    j->planes = (int8_t *)malloc((size_t)d.n_bin * 2 * d.N);
    j->rep = (int8_t *)malloc((size_t)d.n_prn * ML);
    j->grid = grid ? grid : (uint64_t *)malloc(cells * sizeof(uint64_t));
    if (!j->planes || !j->rep || !j->grid) {
        rc = gss_fail(GSS_E_NOMEM, "out of memory (acquisition)");
        goto done;
    }
    gss_lut(j->lut_s, j->lut_c);
    j->sh = a->qshift;
    if (j->sh < 0) {
        int32_t mi = 0, mq = 0;
        for (int64_t n = 0; n < d.N; n++) {
            int32_t xi, xq;
            gss_acq_sample(samples, a->fmt, n, &xi, &xq);
            xi = xi < 0 ? -xi : xi;
            xq = xq < 0 ? -xq : xq;
            mi = xi > mi ? xi : mi;
            mq = xq > mq ? xq : mq;
        }
        j->sh = gss_acq_auto_shift(mi, mq);
    }
    if (qshift_out)
        *qshift_out = j->sh;
    {
        uint32_t ca[32 * GSS_CA_WORDS];
        gss_ca_table(ca);
        for (size_t i = 0; i < ML; i++) {
            const int32_t chip = gss_acq_chip_idx((int64_t)i, a->fs_hz);
            for (int p = 0; p < d.n_prn; p++)
                j->rep[(size_t)p * ML + i] =
                    (int8_t)gss_acq_replica(ca + (size_t)(d.prn[p] - 1) * GSS_CA_WORDS, chip);
        }
    }
    if ((rc = gss_pool_run(threads, d.n_bin, wipe_part, j)) != 0 ||
        (rc = gss_pool_run(threads, d.n_bin * d.n_prn, corr_part, j)) != 0 ||
        (rc = gss_pool_run(threads, d.n_prn, peak_part, j)) != 0)
        goto done;
done:
    free(j->planes);
    free(j->rep);
    if (!grid)
        free(j->grid);
    free(j);
    return rc;
}

int gss_acq_expect(const gss_chan_blk_t *row, double fs, int64_t sample_in_block,
                   gss_acq_truth_t *out)
{
    if (!row || !out || !(fs > 0) || !(row->code_step > 0) || sample_in_block < 0)
        return gss_fail(GSS_E_ARG, "invalid acquisition-label arguments");
    const double code = row->code0 + (double)sample_in_block * row->code_step;
    const double period = 1023.0 / row->code_step;
    double tau = fmod((1023.0 - code) / row->code_step, period);
    if (tau < 0)
        tau += period;
    out->tau = tau;
    out->doppler_hz = row->carr_step * fs;
    out->cn0_offset_db = row->gain > 0 ? 20.0 * log10(row->gain / 128.0) : -INFINITY;
    out->prn = row->ca_tbl + 1;
    out->pad = 0;
    return 0;
}

/* ln(e^-x sum_{j < M} x^j / j!), by the largest term */
static double log_tail(int M, double x)
{
    const double lx = log(x);
    double mx = -INFINITY;
    for (int j = 0; j < M; j++) {
        const double t = -x + j * lx - lgamma(j + 1.0);
        mx = t > mx ? t : mx;
    }
    double s = 0;
    for (int j = 0; j < M; j++)
        s += exp(-x + j * lx - lgamma(j + 1.0) - mx);
    return mx + log(s);
}

double gss_acq_threshold(int M, uint64_t cells, double pfa)
{
    if (M < 1 || M > GSS_ACQ_MMAX || cells < 1 || !(pfa > 0) || !(pfa < 1))
        return NAN;
    const double target = log(pfa / (double)cells);
    double lo = 1e-300, hi = M;
    while (log_tail(M, hi) > target)
        hi *= 2;
    for (int it = 0; it < 200 && hi - lo > 0; it++) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi)
            break;
        if (log_tail(M, mid) > target)
            lo = mid;
        else
            hi = mid;
    }
    return 0.5 * (lo + hi) / M;
}
