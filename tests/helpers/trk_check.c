/*
 * trk_check.c — gss_track_host, gss_nav_decode and gss_trk_cn0 in a stand-alone program for the
 * sanitizers (tools/trk_sanitize.sh builds it with the host sources under -fsanitize=address,
 * undefined and -fsanitize=thread).  Random samples through every format on several threads, a
 * job that runs out of samples, a diverging loop (the wrap-around arithmetic), the argument
 * errors, the limits of the code step with the longest epoch they admit, jobs that end exactly
 * where the samples do, and the decoder on random prompt sums, long and short.  Prints "ok".
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

static size_t bytes_of(int fmt, int64_t N)
{
    return fmt == 16 ? (size_t)N * 4 : fmt == 8 ? (size_t)N * 2 : (size_t)(N + 3) / 4;
}

/* The limits of the code step at 2 GS/s: the configuration whose second epoch would need 2.8e9
   samples is rejected, as is the first Kd beyond the bound; with the last Kd inside it, w0 =
   -2^31 and both bits of an SC01 sample the late chip times the carrier's sign, the early
   envelope is nearly empty, the code step falls close to its floor M >> 23 and the second epoch
   is the longest the calls admit, just below 2^23 samples. */
static int limits(void)
{
    const int32_t fs = 2000000000;
    const int64_t M = 1023LL << 32, cn = (1023000LL * 4294967296LL + fs / 2) / fs;
    const int64_t cs0 = cn - 2147483648LL / 1540;
    const int64_t N = (M + cs0 - 1) / cs0 + (1 << 23);
    gss_trk_cfg_t cfg = {fs, 1, 0, 0, 0, 0, 0};
    gss_trk_job_t job = {0, 1, INT32_MIN, 2, 0};
    gss_trk_rec_t rec[4];
    int32_t count = -1;
    uint32_t ca[32 * GSS_CA_WORDS];
    CHECK(gss_ca_table(ca) == 0);
    uint8_t *x = (uint8_t *)calloc(bytes_of(1, N), 1);
    CHECK(x);
    for (int64_t i = 0; i < N; i++) {
        const int64_t c = (i * cs0 - (1LL << 31)) % M, chip = (c < 0 ? c + M : c) >> 32;
        if (((ca[chip >> 5] >> (chip & 31)) & 1u) != (uint32_t)(i & 1))
            x[i >> 2] |= (uint8_t)(0xC0 >> (2 * (i & 3)));
    }
    cfg.fmt = 8;
    cfg.Kd = 3209600;                                  /* cs_nom - span = 3 */
    job.n_epoch = 4;
    CHECK(gss_track_host(&cfg, x, 1000, &job, 1, rec, 4, &count, 1) == GSS_E_ARG);
    cfg.fmt = 1;
    job.n_epoch = 2;
    cfg.Kd = (int32_t)(4 * (cn - (2147483648LL / 1540 + 2) - 2 - (M >> 23) - 1) + 3);
    cfg.Kd++;
    CHECK(gss_track_host(&cfg, x, N, &job, 1, rec, 4, &count, 1) == GSS_E_ARG);
    cfg.Kd--;
    CHECK(gss_track_host(&cfg, x, N, &job, 1, rec, 4, &count, 1) == 0);
    CHECK(count == 2 && rec[1].s == (M + cs0 - 1) / cs0);
    job.s0 = INT64_MAX;                                /* s0 + an epoch would leave int64 */
    CHECK(gss_track_host(&cfg, x, N, &job, 1, rec, 4, &count, 1) == GSS_E_ARG);
    job.s0 = 1LL << 62;
    CHECK(gss_track_host(&cfg, x, N, &job, 1, rec, 4, &count, 1) == 0 && count == 0);
    CHECK(cn + rec[1].dcs > (M >> 23) && cn + rec[1].dcs < (M >> 23) + 1200);
    free(x);
    return 0;
}

/* Jobs at the end of the samples, the buffer exactly the bytes the call may read: N from a first
   run so that job 0's 40th epoch ends at N, then N - 1 .. N - 3 (every N % 4; 39 epochs); starts
   at every s0 % 4, at N - 1, N and far behind N; n_epoch 0 and 1; the pitch above every n_epoch */
static int ends(int32_t fs, int fmt)
{
    const int32_t T = (fs + 999) / 1000;
    const int64_t N0 = 42 * (int64_t)T + 16;
    uint8_t *x0 = (uint8_t *)malloc(bytes_of(fmt, N0));
    gss_trk_rec_t *rec = (gss_trk_rec_t *)malloc(9 * 64 * sizeof *rec);
    CHECK(x0 && rec);
    for (size_t i = 0; i < bytes_of(fmt, N0); i++)
        x0[i] = (uint8_t)rnd();
    gss_trk_cfg_t cfg;
    CHECK(gss_trk_defaults(fs, fmt, &cfg) == 0);
    cfg.n_pull = 3;
    gss_trk_job_t jobs[9];
    int32_t count[9];
    memset(jobs, 0, sizeof jobs);
    jobs[0].s0 = 4;
    jobs[0].prn = 3;
    jobs[0].w0 = 12345678;
    jobs[0].n_epoch = 41;
    CHECK(gss_track_host(&cfg, x0, N0, jobs, 1, rec, 64, count, 1) == 0 && count[0] == 41);
    const int64_t N1 = rec[40].s;
    for (int k = 0; k < 4; k++) {
        const int64_t N = N1 - k;
        uint8_t *x = (uint8_t *)malloc(bytes_of(fmt, N));
        CHECK(x);
        memcpy(x, x0, bytes_of(fmt, N));
        for (int j = 0; j < 9; j++) {
            jobs[j].prn = 3 + j;
            jobs[j].w0 = j & 1 ? -12345678 : 12345678;
            jobs[j].n_epoch = 40;
            jobs[j].s0 = 4 + j;                        /* 0 .. 3: every s0 % 4 */
        }
        jobs[4].s0 = N - 1;
        jobs[5].s0 = N;
        jobs[6].s0 = N + 1000000;
        jobs[7].n_epoch = 0;
        jobs[8].n_epoch = 1;
        CHECK(gss_track_host(&cfg, x, N, jobs, 9, rec, 64, count, 3) == 0);
        CHECK(count[0] == (k ? 39 : 40) && count[1] >= 38 && count[2] >= 38 && count[3] >= 38);
        CHECK(count[4] == 0 && count[5] == 0 && count[6] == 0 && count[7] == 0 && count[8] == 1);
        free(x);
    }
    free(rec);
    free(x0);
    return 0;
}

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

    if (limits() || ends(64000, 16) || ends(5121000, 16) || ends(64000, 1) || ends(5121000, 1))
        return 1;

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
