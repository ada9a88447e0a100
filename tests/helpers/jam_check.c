/*
 * jam_check.c — gss_jam_host and gss_jam_make as a stand-alone program, for the sanitizers
 * (tools/jam_sanitize.sh builds it with the host sources under -fsanitize=address,undefined).
 * Every buffer is allocated with exactly the bytes the call may touch, so a read or write past
 * either end is an AddressSanitizer report.  Checked besides: the closed form of the definition
 * sample by sample (zero input, no noise, SC16), ranges in two pieces against one, n_jam = 0
 * against gss_impair_host, and the argument errors.  Test infrastructure only.
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

static size_t out_bytes(size_t n, int fmt) { return fmt == 16 ? n * 4 : fmt == 8 ? n * 2 : n / 4; }

/* gss_jam_host into a fresh buffer of exactly the output's bytes, from a copy of iq of exactly
   the input's */
static uint8_t *run(const gss_impair_t *p, const gss_jam_t *jam, int nj, const int16_t *iq,
                    uint64_t s0, size_t n, int fmt)
{
    int16_t *in = malloc(n * 4 ? n * 4 : 1);
    uint8_t *out = malloc(out_bytes(n, fmt) ? out_bytes(n, fmt) : 1);
    memcpy(in, iq, n * 4);
    const int rc = gss_jam_host(p, jam, nj, in, s0, n, fmt, out);
    if (rc) {
        printf("gss_jam_host: %d %s\n", rc, gss_last_error());
        fails++;
    }
    free(in);
    return out;
}

/* the definition in closed form: jI, jQ of sample n */
static void closed(const gss_jam_t *j, uint64_t n, const int32_t *c512, const int32_t *s512,
                   int32_t *ji, int32_t *jq)
{
    const uint64_t P = j->sweep, k = n / P, m = n % P;
    const uint64_t phip = P * j->step0 + j->rate * (P * (P - 1) / 2);
    const uint64_t phi = j->phase0 + k * phip + m * j->step0 + j->rate * (m ? m * (m - 1) / 2 : 0);
    const int on = j->gate_period == 0 ||
                   ((n % j->gate_period) + j->gate_shift) % j->gate_period < j->gate_on;
    const int idx = (int)(phi >> 55);
    *ji = on ? ((int32_t)j->amp * c512[idx] + 32768) >> 16 : 0;
    *jq = on ? ((int32_t)j->amp * s512[idx] + 32768) >> 16 : 0;
}

int main(void)
{
    int32_t s512[512], c512[512];
    CHECK(gss_lut(s512, c512) == 0);
    const size_t N = 4100;
    int16_t *iq = malloc(N * 4), *zero = calloc(N, 4);
    for (size_t i = 0; i < 2 * N; i++)
        iq[i] = (int16_t)((int)((uint32_t)(i * 2654435761u) >> 20) % 4095 - 2047);
    iq[0] = -32768;
    iq[2 * N - 1] = 32767;

    gss_jam_t jam[GSS_MAXJAM];
    CHECK(gss_jam_make(1.0e6, 0.0, 137.0e3, 0.0, 0.0, 0.0, 0.0, &jam[0]) == 0);
    CHECK(jam[0].sweep == 1 && jam[0].rate == 0 && jam[0].amp == 65536 && jam[0].gate_period == 0);
    CHECK(jam[0].step0 == (uint64_t)(int64_t)floor(137.0e3 / 1.0e6 * 18446744073709551616.0 + 0.5));
    CHECK(gss_jam_make(1.0e6, 10.0, -400.0e3, 400.0e3, 137.0e-6, 10.0e-6, 0.3, &jam[1]) == 0);
    CHECK(jam[1].sweep == 137 && jam[1].gate_period == 10 && jam[1].gate_on == 3);
    CHECK(gss_jam_make(2.6e6, 42.1, -1.0e6, 1.0e6, 1.0, 0.0, 0.0, &jam[2]) == 0);
    CHECK(jam[2].sweep == 2600000);
    CHECK(gss_jam_make(1.0e6, 20.0, 1.0, 2.0, 4294.967295, 0.0, 0.0, &jam[3]) == 0);
    CHECK(jam[3].sweep == 4294967295u);
    jam[3].rate = 0x2000000000000007ull;               /* the step passes 2^63 inside a sweep */
    jam[3].gate_period = 3; jam[3].gate_on = 2; jam[3].gate_shift = 1;
    gss_jam_t tmp;
    CHECK(gss_jam_make(1.0e6, 42.2, 0.0, 0.0, 0.0, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 500.0e3, 0.0, 0.0, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 0.0, -500.0e3, 1.0e-3, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 0.0, 1.0, 1.0e-9, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 0.0, 1.0, 5000.0, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 0.0, 0.0, 0.0, 1.0e-3, 1.5, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 0.0, 0.0, 0.0, 1.0e-9, 0.5, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, NAN, 0.0, 0.0, 0.0, 0.0, 0.0, &tmp) == GSS_E_ARG);
    CHECK(gss_jam_make(1.0e6, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, NULL) == GSS_E_ARG);

    const gss_impair_t quiet = {0, 0, 0}, noisy = {0x123456789abcdefull, 256 * 300, 1};
    const uint64_t starts[] = {0, 1, 0xFFFFFFFFull - 4, (1ull << 40) + 3, 0 - (uint64_t)N - 1,
                               5ull * 137 - 3, 5ull * 4294967295ull - 3};
    /* the closed form, every jammer alone (P = 1 among them), across 2^32 and the sweeps' ends */
    for (size_t si = 0; si < sizeof starts / sizeof *starts; si++)
        for (int q = 0; q < GSS_MAXJAM; q++) {
            uint8_t *o = run(&quiet, &jam[q], 1, zero, starts[si], N, 16);
            const int16_t *v = (const int16_t *)o;
            int bad = 0;
            for (size_t i = 0; i < N; i++) {
                int32_t ji, jq;
                closed(&jam[q], starts[si] + i, c512, s512, &ji, &jq);
                ji = ji > 32767 ? 32767 : ji < -32768 ? -32768 : ji;
                jq = jq > 32767 ? 32767 : jq < -32768 ? -32768 : jq;
                bad += v[2 * i] != ji || v[2 * i + 1] != jq;
            }
            CHECK(bad == 0);
            free(o);
        }
    /* every format, with and without noise, 0 / 1 / 4 jammers: two pieces equal one */
    const int fmts[] = {16, 8, 1};
    const size_t sizes[] = {4, 36, 4100};
    for (int f = 0; f < 3; f++)
        for (int z = 0; z < 2; z++)
            for (int nj = 0; nj <= GSS_MAXJAM; nj += nj ? 3 : 1)
                for (size_t zi = 0; zi < 3; zi++)
                    for (size_t si = 0; si < sizeof starts / sizeof *starts; si++) {
                        const gss_impair_t *p = z ? &noisy : &quiet;
                        const size_t n = sizes[zi], cut = n / 2 & ~(size_t)3;
                        const uint64_t s0 = starts[si] + (N - n);      /* ends where N would */
                        uint8_t *whole = run(p, jam, nj, iq, s0, n, fmts[f]);
                        uint8_t *a = run(p, jam, nj, iq, s0, cut, fmts[f]);
                        uint8_t *b = run(p, jam, nj, iq + 2 * cut, s0 + cut, n - cut, fmts[f]);
                        CHECK(memcmp(whole, a, out_bytes(cut, fmts[f])) == 0);
                        CHECK(memcmp(whole + out_bytes(cut, fmts[f]), b,
                                     out_bytes(n - cut, fmts[f])) == 0);
                        if (nj == 0) {
                            uint8_t *w = malloc(out_bytes(n, fmts[f]));
                            CHECK(gss_impair_host(p, iq, s0, n, fmts[f], w) == 0);
                            CHECK(memcmp(whole, w, out_bytes(n, fmts[f])) == 0);
                            free(w);
                        }
                        free(whole); free(a); free(b);
                    }
    /* in place, SC16 */
    {
        int16_t *buf = malloc(N * 4);
        memcpy(buf, iq, N * 4);
        uint8_t *w = run(&noisy, jam, 4, iq, 77, N, 16);
        CHECK(gss_jam_host(&noisy, jam, 4, buf, 77, N, 16, buf) == 0);
        CHECK(memcmp(buf, w, N * 4) == 0);
        free(buf); free(w);
    }
    /* argument errors: nothing is written */
    {
        uint8_t out[64];
        memset(out, 0xA5, sizeof out);
        gss_jam_t b = jam[0];
        b.sweep = 0;
        CHECK(gss_jam_host(&quiet, &b, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        b = jam[0]; b.amp = (1u << 23) + 1;
        CHECK(gss_jam_host(&quiet, &b, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        b = jam[0]; b.gate_period = 4; b.gate_on = 5;
        CHECK(gss_jam_host(&quiet, &b, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        b = jam[0]; b.gate_period = 4; b.gate_shift = 4;
        CHECK(gss_jam_host(&quiet, &b, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        b = jam[0]; b.gate_shift = 1;
        CHECK(gss_jam_host(&quiet, &b, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        b = jam[0]; b.pad = 1;
        CHECK(gss_jam_host(&quiet, &b, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        CHECK(gss_jam_host(&quiet, jam, 5, iq, 0, 8, 16, out) == GSS_E_ARG);
        CHECK(gss_jam_host(&quiet, jam, -1, iq, 0, 8, 16, out) == GSS_E_ARG);
        CHECK(gss_jam_host(&quiet, NULL, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        CHECK(gss_jam_host(NULL, jam, 1, iq, 0, 8, 16, out) == GSS_E_ARG);
        CHECK(gss_jam_host(&quiet, jam, 1, iq, 0, 6, 1, out) == GSS_E_ARG);
        CHECK(gss_jam_host(&quiet, jam, 1, iq, 0, 8, 8, iq) == GSS_E_ARG);
        CHECK(gss_jam_host(&quiet, jam, 1, iq, 0 - 4ull, 8, 16, out) == GSS_E_ARG);
        for (size_t i = 0; i < sizeof out; i++)
            CHECK(out[i] == 0xA5);
        CHECK(gss_jam_host(&quiet, NULL, 0, iq, 0, 8, 16, out) == 0);
    }
    free(iq); free(zero);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("jam_check ok\n");
    return 0;
}
