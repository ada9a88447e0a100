/*
 * gss_echo.h — the multipath echoes as host/device functions, exact integer arithmetic
 * (include/gpssim_amd.h, gss_echo_t).  The same code runs in the GPU kernels
 * (csrc/hip/gss_echo.hip) and in the host statement gss_echo_host (csrc/host/echo.c);
 * tests/echo_oracle.py holds an independent restatement with Python integers.
 *
 *   row      the integers of one live pair (echo, channel row) of a block, from the row's doubles
 *            by exact operations only: scaling by a power of two, trunc, floor, one addition and
 *            the conversion.  The echo's own phase terms are folded in: the carrier phase of
 *            sample s of the block is pb + s ps (mod 2^64) with pb = P0 + theta0 + base dstep
 *            (base: the absolute index of the block's first sample) and ps = Ps + dstep
 *   seed     the state of sample s from its index: X = X0 + s Cs (one 64-bit multiply), q = X >>
 *            32, which fits 32 bits, split by 1023 into the chip and the code period, and the
 *            data bit of that period
 *   next     the state of sample s + 1: X += Cs, the chip moves by what q moved and wraps at 1023
 *            into the code period; the data bit is read again only when the period changed
 *   value    d c (cos, sin) of table cell phi >> 55, times g
 * The table is the packed carrier table of gss_jam.h: cos in the low half of a dword, sin in the
 * high half.  X is kept mod 2^64 (unsigned arithmetic), its shifts are arithmetic, so q = X >> 32
 * always fits 32 bits: a block that would count 2^31 chips or more from its frame's start wraps
 * there, in the header's int64 statement as here (include/gpssim_amd.h states the range).
 */
#ifndef GSS_ECHO_H
#define GSS_ECHO_H

#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_jam.h"

#define GSS_ECHO_HD GSS_JAM_HD
#define GSS_ECHO_ALPHA_MAX (4u << 16)
#define GSS_ECHO_DELAY_END ((uint64_t)GSS_CA_LEN << 32)

typedef struct gss_echo_row {
    uint64_t pb, ps;         /* carrier phase of the block's sample 0, and its step             */
    uint64_t x0, cs;         /* X0 and Cs (two's complement)                                    */
    int32_t g;               /* the pair's gain, -32767..32767                                  */
    int32_t ca_tbl, nav_tbl;
    int32_t pad;
} gss_echo_row_t;            /* 48 bytes */

typedef struct gss_echo_state {
    uint64_t x, phi;
    int32_t chip, cp;        /* q mod 1023 and q div 1023 (floored; cp may be negative)         */
    int32_t dg;              /* d g                                                             */
} gss_echo_state_t;

/* The integers of (echo e, row r) in a block whose first sample has absolute index base; 0 when
   the pair is not live (another PRN, a table index outside its table, a double outside the range
   in which the conversions below are defined; a NaN fails every comparison) or adds nothing
   (g == 0) */
GSS_ECHO_HD int gss_echo_row(const gss_echo_t *e, const gss_chan_blk_t *r, uint64_t base, int n_ca,
                             int n_nav, gss_echo_row_t *o)
{
    if (r->ca_tbl < 0 || r->ca_tbl >= n_ca || r->nav_tbl < 0 || r->nav_tbl >= n_nav)
        return 0;
    if (e->prn != 0 && e->prn != r->ca_tbl + 1)
        return 0;
    if (!(r->carr0 >= 0.0 && r->carr0 <= 1.0 && r->carr_step > -1.0 && r->carr_step < 1.0 &&
          r->code0 >= 0.0 && r->code0 < 1023.0 && r->code_step >= 0.0 && r->code_step < 1024.0))
        return 0;
    int64_t g = ((int64_t)r->gain * (int64_t)e->alpha_q16 + (1 << 15)) >> 16;
    g = g < -32767 ? -32767 : g > 32767 ? 32767 : g;
    if (g == 0)
        return 0;
    const uint64_t p0 = r->carr0 >= 1.0 ? 0u : (uint64_t)(r->carr0 * 18446744073709551616.0);
    const int64_t ph = (int64_t)__builtin_trunc(r->carr_step * 9223372036854775808.0);
    const uint64_t ps = (uint64_t)ph << 1;
    const int64_t c0 = (int64_t)__builtin_floor(r->code0 * 4294967296.0);
    const int64_t cs = (int64_t)__builtin_floor(r->code_step * 4294967296.0 + 0.5);
    const int64_t per = (((int64_t)r->iword * 30 + r->ibit) * 20 + r->icode) * GSS_CA_LEN;
    o->pb = p0 + e->theta0 + base * e->dstep;
    o->ps = ps + e->dstep;
    o->x0 = ((uint64_t)per << 32) + (uint64_t)c0 - e->delay;
    o->cs = (uint64_t)cs;
    o->g = (int32_t)g;
    o->ca_tbl = r->ca_tbl;
    o->nav_tbl = r->nav_tbl;
    o->pad = 0;
    return 1;
}

/* q = chip + 1023 cp, floored */
GSS_ECHO_HD void gss_echo_split(int32_t q, int32_t *chip, int32_t *cp)
{
    int32_t p = q / GSS_CA_LEN, c = q - p * GSS_CA_LEN;
    if (c < 0) {
        c += GSS_CA_LEN;
        p -= 1;
    }
    *chip = c;
    *cp = p;
}

/* d g of code period cp: the data bit from the row's nav words (nav: [GSS_NAV_WORDS]) */
GSS_ECHO_HD int32_t gss_echo_dg(const gss_echo_row_t *r, const uint32_t *nav, int32_t cp)
{
    const uint32_t bit = (uint32_t)(cp < 0 ? 0 : cp) / 20u;
    const uint32_t w = bit / 30u, pos = bit - w * 30u;
    const uint32_t word = nav[w < (uint32_t)(GSS_NAV_WORDS - 1) ? w : (uint32_t)(GSS_NAV_WORDS - 1)];
    return (word >> (29u - pos)) & 1u ? r->g : -r->g;
}

GSS_ECHO_HD void gss_echo_seed(const gss_echo_row_t *r, const uint32_t *nav, uint32_t s,
                               gss_echo_state_t *st)
{
    st->x = r->x0 + (uint64_t)s * r->cs;
    st->phi = r->pb + (uint64_t)s * r->ps;
    gss_echo_split((int32_t)(st->x >> 32), &st->chip, &st->cp);
    st->dg = gss_echo_dg(r, nav, st->cp);
}

GSS_ECHO_HD void gss_echo_next(const gss_echo_row_t *r, const uint32_t *nav, gss_echo_state_t *st)
{
    const uint64_t x = st->x + r->cs;
    const int32_t dq = (int32_t)((uint32_t)(x >> 32) - (uint32_t)(st->x >> 32));
    st->x = x;
    st->phi += r->ps;
    if ((uint32_t)dq < (uint32_t)GSS_CA_LEN) {           /* every real code step: one wrap at most */
        st->chip += dq;
        if (st->chip >= GSS_CA_LEN) {
            st->chip -= GSS_CA_LEN;
            st->cp += 1;
            st->dg = gss_echo_dg(r, nav, st->cp);
        }
    } else {
        gss_echo_split((int32_t)(x >> 32), &st->chip, &st->cp);
        st->dg = gss_echo_dg(r, nav, st->cp);
    }
}

/* the carrier table's cell of the current sample */
GSS_ECHO_HD uint32_t gss_echo_cell(const gss_echo_state_t *st) { return (uint32_t)(st->phi >> 55); }

/* the pair's contribution to the current sample, added to *ei, *eq; ca: the row's chips
   [GSS_CA_WORDS], cs: the packed carrier table's entry at gss_echo_cell(st) */
GSS_ECHO_HD void gss_echo_add_cell(const gss_echo_state_t *st, const uint32_t *ca, uint32_t cs,
                                   int32_t *ei, int32_t *eq)
{
    const uint32_t chip = (uint32_t)st->chip;
    const int32_t a = (ca[chip >> 5] >> (chip & 31u)) & 1u ? st->dg : -st->dg;
    *ei += a * (int32_t)(int16_t)(cs & 0xFFFFu);
    *eq += a * ((int32_t)cs >> 16);
}

/* ... with lut, the packed carrier table */
GSS_ECHO_HD void gss_echo_add(const gss_echo_state_t *st, const uint32_t *ca, const uint32_t *lut,
                              int32_t *ei, int32_t *eq)
{
    gss_echo_add_cell(st, ca, lut[gss_echo_cell(st)], ei, eq);
}

/* x16 + ((e + 64) >> 7), clamped to int16 */
GSS_ECHO_HD int32_t gss_echo_mix(int32_t x16, int32_t e)
{
    const int32_t y = x16 + ((e + 64) >> 7);
    return y < -32768 ? -32768 : y > 32767 ? 32767 : y;
}

#endif /* GSS_ECHO_H */
