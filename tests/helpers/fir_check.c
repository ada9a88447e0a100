/*
 * fir_check.c — gss_fir_host, gss_fir_check and gss_fir_make as a stand-alone program, for the
 * sanitizers (tools/fir_sanitize.sh builds it with the host sources under
 * -fsanitize=address,undefined).  Every buffer is allocated with exactly the bytes the call may
 * touch, so a read or write past either end is an AddressSanitizer report, and the sums at both
 * ends of int32 must pass the undefined-behaviour checks.  Checked besides: the definition with
 * 64-bit sums, ranges in two pieces against one, and the argument errors.  Test infrastructure
 * only.
 */
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

static size_t out_bytes(size_t n, int fmt) { return fmt == 16 ? 4 * n : fmt == 8 ? 2 * n : n / 4; }

/* the definition with int64 sums into bytes */
static void closed(const gss_fir_t *f, const int16_t *in, const int16_t *halo, size_t n, int fmt,
                   uint8_t *out)
{
    const int T = f->n_taps;
    memset(out, 0, out_bytes(n, fmt));
    for (size_t j = 0; j < n; j++)
        for (int c = 0; c < 2; c++) {
            int64_t acc = 0;
            for (int k = 0; k < T; k++) {
                const int64_t i = (int64_t)j - k;
                const int64_t x = i >= 0 ? in[2 * i + c] : halo ? halo[2 * (T - 1 + i) + c] : 0;
                acc += f->taps[k] * x;
            }
            int64_t v = (acc + 8192) >> 14;
            if (fmt == 16) {
                v = v < -32768 ? -32768 : v > 32767 ? 32767 : v;
                const int16_t w = (int16_t)v;
                memcpy(out + 2 * (2 * j + c), &w, 2);
            } else if (fmt == 8) {
                v >>= 4;
                v = v < -128 ? -128 : v > 127 ? 127 : v;
                out[2 * j + c] = (uint8_t)(int8_t)v;
            } else if (v > 0) {
                out[(2 * j + c) / 8] |= (uint8_t)(0x80u >> ((2 * j + c) % 8));
            }
        }
}

/* taps with sum |h| <= 65535; mode 0: random, 1: all positive at the bound, -1: all negative */
static void make_taps(gss_fir_t *f, int T, int mode)
{
    memset(f, 0, sizeof *f);
    f->n_taps = T;
    if (mode) {
        for (int k = 0; k < T; k++) {
            int m = 65535 / T + (k < 65535 % T);
            m = m > 32767 ? 32767 : m;
            f->taps[k] = (int16_t)(mode * m);
        }
        return;
    }
    int64_t l1;
    int sh = 0;
    int16_t t[GSS_MAXTAP];
    for (int k = 0; k < T; k++)
        t[k] = (int16_t)(rnd() >> 48);
    do {
        l1 = 0;
        for (int k = 0; k < T; k++) {
            f->taps[k] = (int16_t)(t[k] / (1 << sh));
            l1 += abs(f->taps[k]);
        }
        sh++;
    } while (l1 > 65535);
}

static void one(int T, size_t n, int fmt, int mode, int with_halo)
{
    gss_fir_t f;
    make_taps(&f, T, mode);
    CHECK(gss_fir_check(&f) == 0);
    int16_t *in = malloc(n ? 4 * n : 1);
    int16_t *halo = with_halo && T > 1 ? malloc(4 * (size_t)(T - 1)) : NULL;
    uint8_t *got = malloc(out_bytes(n, fmt) ? out_bytes(n, fmt) : 1);
    uint8_t *want = malloc(out_bytes(n, fmt) ? out_bytes(n, fmt) : 1);
    for (size_t i = 0; i < 2 * n; i++)
        in[i] = mode ? (int16_t)-32768 : (int16_t)(rnd() >> 48);
    for (int i = 0; halo && i < 2 * (T - 1); i++)
        halo[i] = mode ? (int16_t)-32768 : (int16_t)(rnd() >> 48);
    CHECK(gss_fir_host(&f, in, halo, n, fmt, got) == 0);
    closed(&f, in, halo, n, fmt, want);
    CHECK(memcmp(got, want, out_bytes(n, fmt)) == 0);
    /* two pieces, the second with the first's last T - 1 inputs as its halo */
    const size_t cut = fmt == 1 ? n / 8 * 4 : n / 2;
    if (cut > 0 && cut < n) {
        int16_t *h2 = T > 1 ? malloc(4 * (size_t)(T - 1)) : NULL;
        for (int i = 0; i < T - 1; i++) {
            const int64_t src = (int64_t)cut - (T - 1) + i;
            for (int c = 0; c < 2; c++)
                h2[2 * i + c] = src >= 0 ? in[2 * src + c]
                                         : halo ? halo[2 * (T - 1 + src) + c] : (int16_t)0;
        }
        uint8_t *a = malloc(out_bytes(cut, fmt)), *b = malloc(out_bytes(n - cut, fmt));
        CHECK(gss_fir_host(&f, in, halo, cut, fmt, a) == 0);
        CHECK(gss_fir_host(&f, in + 2 * cut, h2, n - cut, fmt, b) == 0);
        CHECK(memcmp(a, want, out_bytes(cut, fmt)) == 0);
        CHECK(memcmp(b, want + out_bytes(cut, fmt), out_bytes(n - cut, fmt)) == 0);
        free(a);
        free(b);
        free(h2);
    }
    free(in);
    free(halo);
    free(got);
    free(want);
}

int main(void)
{
    static const int Ts[] = {1, 2, 3, 31, 63, 64};
    static const size_t ns[] = {0, 4, 8, 32, 60, 64, 68, 1024, 1028, 4100};
    static const size_t odd[] = {1, 2, 3, 7, 33, 62, 63, 1023, 1025, 4099};
    static const int fmts[] = {16, 8, 1};
    for (int ti = 0; ti < 6; ti++)
        for (int fi = 0; fi < 3; fi++)
            for (int mode = -1; mode <= 1; mode++)
                for (int h = 0; h < 2; h++) {
                    for (int ni = 0; ni < 10; ni++)
                        one(Ts[ti], ns[ni], fmts[fi], mode, h);
                    for (int ni = 0; ni < 10 && fmts[fi] != 1; ni++)
                        one(Ts[ti], odd[ni], fmts[fi], mode, h);
                }
    /* gss_fir_make: every odd length at a few widths, and its refusals */
    for (int T = 3; T <= 63; T += 2)
        for (int w = 1; w <= 20; w++) {
            gss_fir_t f;
            CHECK(gss_fir_make(2.0e6, 1.0e5 * w, T, &f) == 0);
            int sum = 0;
            for (int k = 0; k < T; k++) {
                sum += f.taps[k];
                CHECK(f.taps[k] == f.taps[T - 1 - k]);
            }
            CHECK(sum == 16384 && f.n_taps == T && f.pad == 0 && gss_fir_check(&f) == 0);
        }
    gss_fir_t f;
    CHECK(gss_fir_make(1.0e6, 5.0e5, 4, &f) == GSS_E_ARG);
    CHECK(gss_fir_make(1.0e6, 5.0e5, 65, &f) == GSS_E_ARG);
    CHECK(gss_fir_make(1.0e6, 0.0, 63, &f) == GSS_E_ARG);
    CHECK(gss_fir_make(1.0e6, 1.1e6, 63, &f) == GSS_E_ARG);
    CHECK(gss_fir_make(1.0e6, 5.0e5, 63, NULL) == GSS_E_ARG);
    /* the argument errors leave the output as it is */
    make_taps(&f, 3, 0);
    int16_t in[16] = {0};
    uint8_t out[32];
    memset(out, 0x5A, sizeof out);
    gss_fir_t bad = f;
    bad.n_taps = 65;
    CHECK(gss_fir_host(&bad, in, NULL, 8, 16, out) == GSS_E_ARG);
    bad = f;
    bad.pad = 1;
    CHECK(gss_fir_host(&bad, in, NULL, 8, 16, out) == GSS_E_ARG);
    bad = f;
    bad.taps[0] = 32767; bad.taps[1] = 32767; bad.taps[2] = 2;
    CHECK(gss_fir_host(&bad, in, NULL, 8, 16, out) == GSS_E_ARG);
    CHECK(gss_fir_host(&f, in, NULL, 6, 1, out) == GSS_E_ARG);
    CHECK(gss_fir_host(&f, in, NULL, 8, 16, in) == GSS_E_ARG);
    CHECK(gss_fir_host(NULL, in, NULL, 8, 16, out) == GSS_E_ARG);
    for (size_t i = 0; i < sizeof out; i++)
        CHECK(out[i] == 0x5A);
    if (fails) {
        printf("fir_check: %d failures\n", fails);
        return 1;
    }
    printf("fir_check ok\n");
    return 0;
}
