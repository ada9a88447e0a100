/*
 * echo_check.c — gss_echo_host, gss_echo_check and gss_echo_make as a stand-alone program, for
 * the sanitizers (tools/echo_sanitize.sh builds it with the host sources under
 * -fsanitize=address,undefined).  Every buffer is allocated with exactly the bytes the call may
 * touch, so a read or write past either end is an AddressSanitizer report.  Checked besides: the
 * definition sample by sample with divisions (where gss_echo_host carries its state), ranges in
 * two pieces against one, n_echo = 0 and empty blocks, and the argument errors.  Test
 * infrastructure only.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"

static int fails;
#define CHECK(c)                                                                             \
    do {                                                                                     \
        if (!(c)) {                                                                          \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);                              \
            fails++;                                                                         \
        }                                                                                    \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static double unit(void) { return (double)(rnd() >> 11) / 9007199254740992.0; }

static int64_t fdiv(int64_t a, int64_t b) { return a / b - ((a % b) != 0 && ((a < 0) != (b < 0))); }

/* the definition, one sample: E_I, E_Q of block row r under echo e */
static void closed(const gss_echo_t *e, const gss_chan_blk_t *r, const uint32_t *ca,
                   const uint32_t *nav, int64_t s, uint64_t a, const int32_t *c512,
                   const int32_t *s512, int32_t *ei, int32_t *eq)
{
    if (e->prn != 0 && e->prn != r->ca_tbl + 1)
        return;
    if (!(r->carr0 >= 0.0 && r->carr0 <= 1.0 && r->carr_step > -1.0 && r->carr_step < 1.0 &&
          r->code0 >= 0.0 && r->code0 < 1023.0 && r->code_step >= 0.0 && r->code_step < 1024.0))
        return;                                        /* outside the definition's range */
    const uint64_t p0 = r->carr0 >= 1.0 ? 0 : (uint64_t)(r->carr0 * 18446744073709551616.0);
    const uint64_t ps = (uint64_t)(2 * (int64_t)trunc(r->carr_step * 9223372036854775808.0));
    const int64_t c0 = (int64_t)floor(r->code0 * 4294967296.0);
    const int64_t cs = (int64_t)floor(r->code_step * 4294967296.0 + 0.5);
    const int64_t x0 = ((((int64_t)r->iword * 30 + r->ibit) * 20 + r->icode) * 1023) * 4294967296ll +
                       c0 - (int64_t)e->delay;
    int64_t g = ((int64_t)r->gain * (int64_t)e->alpha_q16 + 32768) >> 16;
    g = g < -32767 ? -32767 : g > 32767 ? 32767 : g;
    const int64_t q = (x0 + s * cs) >> 32;
    const int64_t per = fdiv(q, 1023), chip = q - per * 1023, cp = per < 0 ? 0 : per;
    const int64_t bit = cp / 20, word = bit / 30 < 59 ? bit / 30 : 59, pos = bit % 30;
    const int c = (int)((ca[r->ca_tbl * GSS_CA_WORDS + chip / 32] >> (chip % 32)) & 1) * 2 - 1;
    const int d = (int)((nav[r->nav_tbl * GSS_NAV_WORDS + word] >> (29 - pos)) & 1) * 2 - 1;
    const uint64_t phi = p0 + (uint64_t)s * ps + e->theta0 + a * e->dstep;
    *ei += d * c * c512[phi >> 55] * (int32_t)g;
    *eq += d * c * s512[phi >> 55] * (int32_t)g;
}

static int clamp16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

int main(void)
{
    int32_t s512[512], c512[512];
    CHECK(gss_lut(s512, c512) == 0);
    uint32_t *ca = malloc(32 * GSS_CA_WORDS * sizeof *ca);
    CHECK(gss_ca_table(ca) == 0);
    enum { NNAV = 3 };
    uint32_t *nav = malloc(NNAV * GSS_NAV_WORDS * sizeof *nav);
    for (int i = 0; i < NNAV * GSS_NAV_WORDS; i++)
        nav[i] = (uint32_t)rnd() & 0x3FFFFFFFu;
    const double csteps[] = {0.3935, 1.0, 31.9, 1022.5, 1.0 / 131072.0};
    const double dsteps[] = {1.7e-3, -1.1e-3, 0.45, -0.45, 0.0};
    const int sizes[] = {1, 2, 3, 7, 33, 1025};
    const uint64_t starts[] = {0, 1, 4294967291ull, 1099511627779ull};
    /* every delay class on live rows (rows 0, 9, ... are PRN 5); the last one alone when one
       echo is asked for */
    gss_echo_t echo5[5] = {
        {(uint64_t)1 << 31, (uint64_t)1 << 62, (uint64_t)12345 << 20, 32768, 0},
        {((uint64_t)1023 << 32) - 1, 0xF123456789ABCDEFull, (uint64_t)0 - ((uint64_t)777 << 30), 65536, 0},
        {((uint64_t)1 << 32) + 1, 0, 0xF123456789ABCDEFull, 1u << 18, 5},
        {1, 5, 0, 20000, 0},
        {0, 7, (uint64_t)1 << 40, 65536, 0},
    };
    for (unsigned t = 0; t < sizeof sizes / sizeof *sizes; t++) {
        const int n = sizes[t], nblk = 4;
        const int nchs[4] = {16, 0, 5, 1};
        gss_chan_blk_t *blk = calloc((size_t)nblk * GSS_MAXCH, sizeof *blk);
        int32_t *nch = malloc(nblk * sizeof *nch);
        int row = 0;
        for (int b = 0; b < nblk; b++) {
            nch[b] = nchs[b];
            for (int k = 0; k < nchs[b]; k++, row++) {
                gss_chan_blk_t *r = &blk[b * GSS_MAXCH + k];
                r->carr0 = row % 7 == 0 ? 1.0 : unit();
                r->carr_step = dsteps[row % 5];
                r->code0 = row % 3 == 0 ? 0.0 : unit() * 1023.0;
                r->code_step = csteps[row % 5];
                r->icode = row % 3 == 0 ? 0 : row % 4 == 1 ? 19 : (int)(rnd() % 20);
                r->ibit = row % 3 == 0 ? 0 : row % 4 == 1 ? 29 : (int)(rnd() % 30);
                r->iword = row % 3 == 0 ? 0 : row % 4 == 1 ? 59 : (int)(rnd() % 40);
                r->gain = row % 6 == 2 ? 20000 : row % 6 == 3 ? -20000 : (int)(rnd() % 600) - 300;
                r->ca_tbl = row % 9 == 0 ? 4 : (int)(rnd() % 31);
                r->nav_tbl = (int)(rnd() % NNAV);
                if (n == 33 && row % 5 == 4)           /* outside the range: adds nothing */
                    r->code_step = row % 2 ? NAN : 1024.0;
            }
        }
        const size_t N = (size_t)nblk * n;
        int16_t *iq = malloc(N * 4);
        for (size_t i = 0; i < 2 * N; i++)
            iq[i] = (int16_t)(rnd() % 4095) - 2047;
        iq[0] = -32768;
        iq[2 * N - 1] = 32767;
        for (int ne = 0; ne <= 4; ne += ne < 1 ? 1 : 3) {
            const uint64_t s0 = starts[(t + ne) % 4];
            const gss_echo_t *echo = ne == 1 ? echo5 + 4 : echo5;
            int16_t *got = malloc(N * 4);
            memcpy(got, iq, N * 4);
            CHECK(gss_echo_host(echo, ne, blk, nch, nblk, n, ca, 32, nav, NNAV, s0, got) == 0);
            for (size_t i = 0; i < N; i++) {
                const int b = (int)(i / n);
                int32_t ei = 0, eq = 0;
                for (int j = 0; j < ne; j++)
                    for (int k = 0; k < nch[b]; k++)
                        closed(&echo[j], &blk[b * GSS_MAXCH + k], ca, nav, (int64_t)(i % n), s0 + i,
                               c512, s512, &ei, &eq);
                if (got[2 * i] != clamp16(iq[2 * i] + ((ei + 64) >> 7)) ||
                    got[2 * i + 1] != clamp16(iq[2 * i + 1] + ((eq + 64) >> 7))) {
                    printf("FAIL n %d echoes %d sample %zu\n", n, ne, i);
                    fails++;
                    break;
                }
            }
            /* two pieces against one */
            for (int cut = 0; cut <= nblk; cut++) {
                int16_t *a = malloc((size_t)cut * n * 4 ? (size_t)cut * n * 4 : 1);
                int16_t *b = malloc((size_t)(nblk - cut) * n * 4 ? (size_t)(nblk - cut) * n * 4 : 1);
                memcpy(a, iq, (size_t)cut * n * 4);
                memcpy(b, iq + 2 * (size_t)cut * n, (size_t)(nblk - cut) * n * 4);
                CHECK(gss_echo_host(echo, ne, blk, nch, cut, n, ca, 32, nav, NNAV, s0, a) == 0);
                CHECK(gss_echo_host(echo, ne, blk + cut * GSS_MAXCH, nch + cut, nblk - cut, n, ca, 32,
                                    nav, NNAV, s0 + (uint64_t)cut * n, b) == 0);
                CHECK(memcmp(a, got, (size_t)cut * n * 4) == 0);
                CHECK(memcmp(b, got + 2 * (size_t)cut * n, (size_t)(nblk - cut) * n * 4) == 0);
                free(a);
                free(b);
            }
            if (ne == 0)
                CHECK(memcmp(got, iq, N * 4) == 0);
            free(got);
        }
        /* argument errors leave the samples alone */
        {
            const gss_echo_t *echo = echo5;
            int16_t *got = malloc(N * 4);
            memcpy(got, iq, N * 4);
            gss_echo_t bad = echo[0];
            bad.delay = (uint64_t)1023 << 32;
            CHECK(gss_echo_host(&bad, 1, blk, nch, nblk, n, ca, 32, nav, NNAV, 0, got) == GSS_E_ARG);
            bad = echo[0];
            bad.alpha_q16 = (1u << 18) + 1;
            CHECK(gss_echo_host(&bad, 1, blk, nch, nblk, n, ca, 32, nav, NNAV, 0, got) == GSS_E_ARG);
            bad = echo[0];
            bad.prn = 33;
            CHECK(gss_echo_host(&bad, 1, blk, nch, nblk, n, ca, 32, nav, NNAV, 0, got) == GSS_E_ARG);
            CHECK(gss_echo_host(echo, 5, blk, nch, nblk, n, ca, 32, nav, NNAV, 0, got) == GSS_E_ARG);
            CHECK(gss_echo_host(echo, 1, blk, nch, nblk, n, ca, 32, nav, NNAV,
                                (uint64_t)0 - N + 1, got) == GSS_E_ARG);
            nch[0] = 17;
            CHECK(gss_echo_host(echo, 1, blk, nch, nblk, n, ca, 32, nav, NNAV, 0, got) == GSS_E_ARG);
            CHECK(memcmp(got, iq, N * 4) == 0);
            free(got);
        }
        free(iq);
        free(nch);
        free(blk);
    }
    gss_echo_t e;
    CHECK(gss_echo_make(1.0e6, 0, 150.0, 6.0, 30.0, 2.5, &e) == 0 && e.prn == 0 && e.alpha_q16 == 32846);
    CHECK(gss_echo_make(1.0e6, 33, 150.0, 6.0, 0.0, 0.0, &e) == GSS_E_ARG);
    CHECK(gss_echo_make(1.0e6, 1, 3.0e5, 6.0, 0.0, 0.0, &e) == GSS_E_ARG);
    CHECK(gss_echo_make(1.0e6, 1, 150.0, -13.0, 0.0, 0.0, &e) == GSS_E_ARG);
    CHECK(gss_echo_make(1.0e6, 1, 150.0, 6.0, 0.0, 5.0e5, &e) == GSS_E_ARG);
    CHECK(gss_echo_make(1.0e6, 1, 150.0, 6.0, -1e-20, 0.0, &e) == 0 && e.theta0 == 0);
    CHECK(gss_echo_check(NULL, 0) == 0 && gss_echo_check(NULL, 1) == GSS_E_ARG);
    free(nav);
    free(ca);
    if (fails) {
        printf("echo_check: %d failures\n", fails);
        return 1;
    }
    printf("echo_check ok\n");
    return 0;
}
