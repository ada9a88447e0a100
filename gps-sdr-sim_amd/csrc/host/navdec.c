/*
 * navdec.c — what a receiver reads out of the tracking records (gss_trk_rec_t): bit and frame
 * synchronisation with the IS-GPS-200 parity (gss_nav_decode) and the tracked C/N0 by the
 * moments of the prompt power (gss_trk_cn0).  Host only; the parity arithmetic is the
 * producers' (csrc/common/gss_nav.h).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_nav.h"

#define NAV_BIT_EPOCHS 20
#define NAV_SF_BITS    300
#define NAV_PREAMBLE   0x8Bu
#define NAV_DATA_MASK  0x3FFFFFC0u

static int64_t bit_sum(const gss_trk_rec_t *rec, int64_t first)
{
    int64_t a = 0;
    for (int k = 0; k < NAV_BIT_EPOCHS; k++)
        a += rec[first + k].IP;
    return a;
}

/* the subframe whose first bit is b[p] (b[p - 2], b[p - 1] = D29*, D30*), every bit xor pol:
   1 and its words, or 0 */
static int try_subframe(const uint8_t *b, int64_t p, int pol, uint32_t *word)
{
    uint32_t d29 = b[p - 2] ^ (uint32_t)pol, d30 = b[p - 1] ^ (uint32_t)pol;
    for (int w = 0; w < 10; w++) {
        uint32_t R = 0;
        for (int i = 0; i < 30; i++)
            R = R << 1 | (b[p + 30 * w + i] ^ (uint32_t)pol);
        if (w == 0 && (R >> 22) != NAV_PREAMBLE)
            return 0;
        const uint32_t d = (d30 ? R ^ NAV_DATA_MASK : R) & NAV_DATA_MASK;
        if (gss_nav_parity(d | d29 << 31 | d30 << 30, 0) != R)
            return 0;
        word[w] = R;
        d29 = R >> 1 & 1u;
        d30 = R & 1u;
    }
    return 1;
}

int gss_nav_decode(const gss_trk_rec_t *rec, int64_t n, int64_t skip, gss_nav_sf_t *sf, int cap,
                   int32_t *bit_offset)
{
    if (!rec || n < 0 || cap < 0 || (cap > 0 && !sf))
        return gss_fail(GSS_E_ARG, "invalid decoder arguments");
    if (skip < 0)
        skip = 500;
    if (bit_offset)
        *bit_offset = 0;
    const int64_t nb = (n - skip - (NAV_BIT_EPOCHS - 1)) / NAV_BIT_EPOCHS;
    if (n - skip < 2 * NAV_BIT_EPOCHS - 1 || nb < 1)
        return 0;
    int best = 0;
    double best_v = -1.0;
    for (int o = 0; o < NAV_BIT_EPOCHS; o++) {
        double v = 0.0;
        for (int64_t k = 0; k < nb; k++)
            v += fabs((double)bit_sum(rec, skip + o + k * NAV_BIT_EPOCHS));
        if (v > best_v) {
            best_v = v;
            best = o;
        }
    }
    if (bit_offset)
        *bit_offset = best;
    const int64_t first = skip + best, nbits = (n - first) / NAV_BIT_EPOCHS;
    uint8_t *b = (uint8_t *)malloc((size_t)nbits + 1);
    if (!b)
        return gss_fail(GSS_E_NOMEM, "out of memory");
    for (int64_t k = 0; k < nbits; k++)
        b[k] = bit_sum(rec, first + k * NAV_BIT_EPOCHS) >= 0;
    int found = 0;
    for (int64_t p = 2; p + NAV_SF_BITS <= nbits && found < cap;) {
        uint32_t word[10];
        int pol = -1;
        if (try_subframe(b, p, 0, word))
            pol = 0;
        else if (try_subframe(b, p, 1, word))
            pol = 1;
        if (pol < 0) {
            p++;
            continue;
        }
        gss_nav_sf_t *o = &sf[found++];
        o->epoch = (int32_t)(first + p * NAV_BIT_EPOCHS);
        o->sample = rec[o->epoch].s;
        o->polarity = pol;
        /* the hand-over word's data bits are inverted when the word before ends in a one */
        const uint32_t how = (word[0] & 1u) ? word[1] ^ NAV_DATA_MASK : word[1];
        o->tow = (int32_t)(how >> 13 & 0x1FFFFu);
        o->id = (int32_t)(how >> 8 & 7u);
        memcpy(o->word, word, sizeof word);
        p += NAV_SF_BITS;
    }
    free(b);
    return found;
}

double gss_trk_cn0(const gss_trk_rec_t *rec, int64_t n, int64_t skip)
{
    if (!rec || skip < 0 || n - skip < 2)
        return NAN;
    double m2 = 0.0, m4 = 0.0;
    for (int64_t k = skip; k < n; k++) {
        const double i = (double)rec[k].IP, q = (double)rec[k].QP, p = i * i + q * q;
        m2 += p;
        m4 += p * p;
    }
    m2 /= (double)(n - skip);
    m4 /= (double)(n - skip);
    const double x = 2.0 * m2 * m2 - m4;
    if (!(x > 0.0))
        return NAN;
    const double pd = sqrt(x), pn = m2 - pd;
    if (!(pn > 0.0))
        return NAN;
    return 10.0 * log10(pd / pn / 1e-3);
}
