/*
 * pvt_check.c — gss_obs_host, the gss_navdata calls and gss_pvt_solve in a stand-alone program
 * for the sanitizers (tools/pvt_sanitize.sh builds it with the host sources under
 * -fsanitize=address,undefined and -fsanitize=thread and runs it on the CPU).  Every buffer is
 * allocated with exactly the bytes a call may read or write, so a read or write past an end is
 * a report.  Run from the repository's root (it reads tests/golden/data/brdc3540.14n).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, gss_last_error()); \
            return 1;                                                   \
        }                                                               \
    } while (0)

#define M_CODE (1023LL << 32)
#define C_LIGHT 2.99792458e8

/* count records of consistent lengths from sample s0 at fs: only s, w and dcs matter */
static void fill(gss_trk_rec_t *r, int count, int64_t s0, int32_t fs, unsigned seed)
{
    const int64_t cs_nom = (1023000LL * 4294967296LL + fs / 2) / fs;
    int64_t s = s0, phi = 0;
    for (int e = 0; e < count; e++) {
        seed = seed * 1103515245u + 12345u;
        r[e].s = s;
        r[e].w = (int32_t)seed;
        r[e].dcs = (int32_t)(seed >> 20) - 2048;
        const int64_t cs = cs_nom + r[e].dcs, n = (M_CODE - phi + cs - 1) / cs;
        s += n;
        phi += n * cs - M_CODE;
    }
}

static int observables(void)
{
    const int32_t fs = 4000;
    /* pitch == the largest count; jobs of 0, 1, 2 and 900 records; one thread and many */
    const int32_t counts[4] = {0, 1, 2, 900};
    const int64_t pitch = 900;
    for (int threads = 1; threads <= 8; threads += 7) {
        gss_trk_rec_t *rec = (gss_trk_rec_t *)malloc(4 * (size_t)pitch * sizeof *rec);
        int32_t *count = (int32_t *)malloc(sizeof counts);
        CHECK(rec && count);
        memset(rec, 0x5A, 4 * (size_t)pitch * sizeof *rec);
        memcpy(count, counts, sizeof counts);
        for (int j = 0; j < 4; j++)
            fill(rec + j * pitch, counts[j], 10 + j, fs, 7u + (unsigned)j);
        const int32_t n_fix = 1300;
        gss_obs_t *obs = (gss_obs_t *)malloc(4 * (size_t)n_fix * sizeof *obs);
        CHECK(obs);
        CHECK(gss_obs_host(fs, rec, pitch, count, 4, 5, 3, n_fix, obs, threads) == 0);
        for (int k = 0; k < n_fix; k++)
            CHECK(obs[k].epoch == -1 && obs[k].code == 0);
        CHECK(obs[n_fix].epoch == -1 && obs[n_fix + 1].epoch == -1 && obs[n_fix + 2].epoch == 0);
        int seen = 0;
        for (int k = 0; k < n_fix; k++) {
            const gss_obs_t *o = &obs[3 * n_fix + k];
            if (o->epoch >= 0) {
                CHECK(o->code >= 0 && o->code < M_CODE && o->w == rec[3 * pitch + o->epoch].w);
                seen = o->epoch > seen ? o->epoch : seen;
            }
        }
        CHECK(seen == 899 && obs[4 * n_fix - 1].epoch == -1);
        /* no instants: obs is not touched (a NULL is accepted); count 0 everywhere: no record
           is read (a NULL is accepted) */
        CHECK(gss_obs_host(fs, rec, pitch, count, 4, 0, 1, 0, NULL, threads) == 0);
        int32_t zero[2] = {0, 0};
        CHECK(gss_obs_host(fs, NULL, 0, zero, 2, 0, 1, 4, obs, threads) == 0);
        CHECK(obs[7].epoch == -1);
        CHECK(gss_obs_host(fs, rec, pitch, count, 4, 0, 0, 4, obs, threads) == GSS_E_ARG);
        count[1] = 901;
        CHECK(gss_obs_host(fs, rec, pitch, count, 4, 0, 1, 4, obs, threads) == GSS_E_ARG);
        free(rec);
        free(count);
        free(obs);
    }
    return 0;
}

static int fixes(void)
{
    const char *nav = "tests/golden/data/brdc3540.14n";
    gss_navdata *nd = NULL, *empty = NULL;
    CHECK(gss_navdata_open_rinex(&nd, "no/such/file") == GSS_E_IO && nd == NULL);
    CHECK(gss_navdata_open_rinex(&nd, nav) == 0);
    CHECK(gss_navdata_open_empty(&empty) == 0);
    double *f = (double *)malloc(GSS_NAVDATA_FIELDS * sizeof *f);
    CHECK(f && gss_navdata_get(nd, 1, f, GSS_NAVDATA_FIELDS) == 0 && f[0] == 0.0);
    CHECK(gss_navdata_get(nd, 32, f, 1) == 0);
    CHECK(gss_navdata_get(nd, 33, f, 1) == GSS_E_ARG);
    CHECK(gss_navdata_get(nd, 1, f, GSS_NAVDATA_FIELDS + 1) == GSS_E_ARG);
    free(f);
    gss_nav_sf_t *sf = (gss_nav_sf_t *)calloc(1, sizeof *sf);
    CHECK(sf);
    for (int id = 1; id <= 5; id++) {                 /* all-zero words: accepted, complete nothing */
        sf->id = id;
        CHECK(gss_navdata_add_subframe(empty, 5, sf) == 0);
        CHECK(gss_navdata_add_subframe(nd, 5, sf) == 0);
    }
    sf->id = 6;
    CHECK(gss_navdata_add_subframe(empty, 5, sf) == GSS_E_ARG);
    free(sf);

    /* observables of a receiver at a known place, from the model itself */
    const double xyz[3] = {-2758918.635, 4772301.120, 3197889.437};
    const int week = 1823;
    const double sec = 518400.0 + 7200.0, fs = 1.0e6;
    const int64_t t = 1234567;
    gss_pvt_sat_t *sats = (gss_pvt_sat_t *)calloc(32, sizeof *sats);
    CHECK(sats);
    int n = 0;
    for (int prn = 1; prn <= 32; prn++) {
        double out[2];
        if (gss_pvt_range(nd, prn, week, sec + (double)t / fs, xyz, 0, out) != 0)
            continue;
        if (out[0] > 2.45e7)                           /* the far side of the sky */
            continue;
        const long double tx = (long double)sec + (long double)t / fs - (long double)out[0] / C_LIGHT;
        const long double sub = floorl(tx / 6.0L);
        const long double ms = (tx - 6.0L * sub) * 1000.0L;
        const long double e = floorl(ms);
        sats[n].prn = prn;
        sats[n].sf_tow = (int32_t)sub + 1;
        sats[n].sf_epoch = 700;
        sats[n].obs.epoch = 700 + (int32_t)e;
        sats[n].obs.code = (int64_t)((ms - e) * (long double)M_CODE);
        sats[n].obs.w = 1000 * prn;
        n++;
    }
    printf("satellites in view: %d\n", n);
    CHECK(n >= 6);
    gss_pvt_fix_t *fix = (gss_pvt_fix_t *)malloc(sizeof *fix);
    CHECK(fix);
    for (int k = 0; k <= 3; k++) {                     /* fewer than four: a status, buffers exact */
        gss_pvt_sat_t *few = (gss_pvt_sat_t *)malloc((size_t)(k ? k : 1) * sizeof *few);
        CHECK(few);
        memcpy(few, sats, (size_t)k * sizeof *few);
        CHECK(gss_pvt_solve(nd, fs, t, k ? few : NULL, k, NULL, fix) == 0);
        CHECK(fix->status == GSS_PVT_FEW && fix->n_used == k);
        free(few);
    }
    CHECK(gss_pvt_solve(empty, fs, t, sats, n, NULL, fix) == 0 && fix->status == GSS_PVT_FEW);
    gss_pvt_sat_t *exact = (gss_pvt_sat_t *)malloc((size_t)n * sizeof *exact);
    CHECK(exact);
    memcpy(exact, sats, (size_t)n * sizeof *exact);
    CHECK(gss_pvt_solve(nd, fs, t, exact, n, NULL, fix) == 0 && fix->status == GSS_PVT_OK);
    const double d = sqrt(pow(fix->xyz[0] - xyz[0], 2) + pow(fix->xyz[1] - xyz[1], 2) +
                          pow(fix->xyz[2] - xyz[2], 2));
    printf("fix: %d satellites, %.3g m from the truth, T0 off by %.3g s, pdop %.2f\n", fix->n_used,
           d, fix->t0_sec - sec, fix->pdop);
    CHECK(fix->n_used == n && d < 1e-3 && fabs(fix->t0_sec - sec) < 1e-9 && fix->t0_week == week);
    for (int i = 0; i < n; i++)                        /* one direction five times: no geometry */
        exact[i] = sats[0];
    CHECK(gss_pvt_solve(nd, fs, t, exact, n, NULL, fix) == 0 && fix->status != GSS_PVT_OK);
    CHECK(gss_pvt_solve(nd, 0.0, t, exact, n, NULL, fix) == GSS_E_ARG);
    free(exact);
    free(fix);
    free(sats);
    CHECK(gss_navdata_close(nd) == 0 && gss_navdata_close(empty) == 0);
    return 0;
}

int main(void)
{
    if (observables() || fixes())
        return 1;
    printf("pvt_check ok\n");
    return 0;
}
