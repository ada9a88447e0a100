/*
 * trk_check.c — gss_track_host, gss_nav_decode and gss_trk_cn0 in a stand-alone program for the
 * sanitizers (tools/trk_sanitize.sh builds it with the host sources under -fsanitize=address,
 * undefined and -fsanitize=thread).  Random samples through every format on several threads, a
 * job that runs out of samples, a diverging loop (the wrap-around arithmetic), the argument
 * errors, and the decoder on random prompt sums, long and short.  Prints "ok".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"

static uint64_t rng = 88172645463325252ull;
static uint32_t rnd(void)
{
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)(rng >> 16);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, \
                                          gss_last_error()); return 1; } } while (0)

int main(void)
{
    const int32_t rates[3] = {64000, 100010, 2600000};
    const int fmts[3] = {16, 8, 1};
    for (int r = 0; r < 3; r++)
        for (int f = 0; f < 3; f++) {
            const int32_t fs = rates[r], T = (fs + 999) / 1000, ne = 40;
            const int64_t N = (int64_t)ne * fs / 1000 + T + 7;
            const size_t nb = fmts[f] == 16 ? (size_t)N * 4 : fmts[f] == 8 ? (size_t)N * 2
                                                                          : (size_t)(N + 3) / 4;
            uint8_t *x = (uint8_t *)malloc(nb);        /* exactly the bytes the call may read */
            CHECK(x);
            for (size_t i = 0; i < nb; i++)
                x[i] = (uint8_t)rnd();
            gss_trk_cfg_t cfg;
            CHECK(gss_trk_defaults(fs, fmts[f], &cfg) == 0);
            cfg.n_pull = 15;
            if (r == 0) {                              /* a loop that diverges: W and w wrap */
                cfg.Kf = cfg.Ki = cfg.Kp = 1 << 30;
                cfg.Kd = 1 << 20;
            }
            gss_trk_job_t jobs[5];
            for (int j = 0; j < 5; j++) {
                jobs[j].s0 = j < 4 ? (int64_t)(rnd() % (uint32_t)T) : N - 5 * (int64_t)T;
                jobs[j].prn = 1 + (int32_t)(rnd() % 32);
                jobs[j].w0 = (int32_t)rnd();
                jobs[j].n_epoch = ne - j;
                jobs[j].pad = 0;
            }
            gss_trk_rec_t *rec = (gss_trk_rec_t *)malloc(5 * (size_t)ne * sizeof *rec);
            int32_t count[5];
            CHECK(rec);
            CHECK(gss_track_host(&cfg, x, N, jobs, 5, rec, ne, count, 4) == 0);
            CHECK(count[0] == ne && count[4] > 0 && count[4] < ne - 4);
            gss_nav_sf_t sf[4];
            int32_t off;
            CHECK(gss_nav_decode(rec, count[0], 0, sf, 4, &off) >= 0);
            (void)gss_trk_cn0(rec, count[0], 0);
            jobs[0].prn = 33;
            CHECK(gss_track_host(&cfg, x, N, jobs, 5, rec, ne, count, 4) == GSS_E_ARG);
            free(rec);
            free(x);
        }

    /* the decoder on 620 random bits (parity fails everywhere, so every position is tried in
       both polarities) and on streams shorter than two bits: none may read outside its records */
    const int n = 500 + 7 + 20 * 620;
    gss_trk_rec_t *rec = (gss_trk_rec_t *)calloc((size_t)n, sizeof *rec);
    CHECK(rec);
    for (int k = 0; k < n; k++) {
        rec[k].IP = (rnd() & 1) ? 1000 : -1000;
        rec[k].QP = (int64_t)(rnd() % 200) - 100;
        rec[k].s = 1000 * (int64_t)k;
    }
    gss_nav_sf_t sf[8];
    int32_t off = -1;
    CHECK(gss_nav_decode(rec, n, -1, sf, 8, &off) == 0 && off >= 0 && off < 20);
    CHECK(gss_nav_decode(rec, 520, -1, sf, 8, &off) == 0);
    CHECK(gss_nav_decode(rec, 0, -1, sf, 8, NULL) == 0);
    CHECK(gss_nav_decode(NULL, n, -1, sf, 8, NULL) == GSS_E_ARG);
    (void)gss_trk_cn0(rec, n, 500);
    free(rec);
    printf("ok\n");
    return 0;
}
