/*
 * gss_jam.h — the jammers as host/device functions, exact integer arithmetic mod 2^64
 * (include/gpssim_amd.h, gss_jam_t).  The same code runs in the GPU kernels
 * (csrc/hip/gss_jam.hip) and in the host statement gss_jam_host (csrc/host/jam.c);
 * tests/jam_oracle.py holds an independent restatement with Python integers.
 *
 *   seed     the state of sample n from its index: one 64-by-32-bit division gives (k, m) =
 *            (n div P, n mod P), from them Phi = phase0 + k PhiP + m step0 + rate m (m - 1) / 2
 *            and the current step step0 + m rate; one more division places the gate
 *   next     the state of sample n + 1: Phi += step, step += rate, m += 1, and at m == P the
 *            sweep starts again (m = 0, step = step0); the phase needs no correction there,
 *            because k PhiP is by definition what P such additions come to
 *   value    (cos, sin) of table cell Phi >> 55, scaled: (amp c + 2^15) >> 16, or 0 off-gate
 * The table is the carrier table of gss_lut, one dword per cell: cos in the low half, sin in the
 * high half (both int16).
 */
#ifndef GSS_JAM_H
#define GSS_JAM_H

#include <stdint.h>
#include "gpssim_amd.h"

#if defined(__HIPCC__)
#define GSS_JAM_HD __host__ __device__ inline
#else
#define GSS_JAM_HD static inline
#endif

#define GSS_JAM_LUT 512                  /* cells of the packed carrier table */
#define GSS_JAM_AMP_MAX (1u << 23)

typedef struct gss_jam_state {
    uint64_t phi;                        /* Phi of the current sample                      */
    uint64_t step;                       /* what the next sample adds to it                */
    uint32_t m;                          /* n mod P                                        */
    uint32_t g;                          /* ((n mod gate_period) + gate_shift) mod gate_period */
} gss_jam_state_t;

/* x (x - 1) / 2 for x < 2^32: the product is below 2^64, so the half is exact */
GSS_JAM_HD uint64_t gss_jam_tri(uint32_t x)
{
    return x ? ((uint64_t)x * (uint64_t)(x - 1u)) >> 1 : 0;
}

/* one packed table cell from the two tables' entries */
GSS_JAM_HD uint32_t gss_jam_cell(int32_t c, int32_t s)
{
    return ((uint32_t)c & 0xFFFFu) | ((uint32_t)s << 16);
}

GSS_JAM_HD void gss_jam_seed(const gss_jam_t *j, uint64_t n, gss_jam_state_t *st)
{
    const uint32_t P = j->sweep;
    if (P == 1) {                        /* k = n, m = 0, PhiP = step0 */
        st->m = 0;
        st->step = j->step0;
        st->phi = j->phase0 + n * j->step0;
    } else {
        const uint64_t k = n / P;
        const uint32_t m = (uint32_t)(n - k * P);
        const uint64_t phip = (uint64_t)P * j->step0 + j->rate * gss_jam_tri(P);
        st->m = m;
        st->step = j->step0 + (uint64_t)m * j->rate;
        st->phi = j->phase0 + k * phip + (uint64_t)m * j->step0 + j->rate * gss_jam_tri(m);
    }
    st->g = j->gate_period
                ? (uint32_t)((n % j->gate_period + j->gate_shift) % j->gate_period) : 0u;
}

GSS_JAM_HD void gss_jam_next(const gss_jam_t *j, gss_jam_state_t *st)
{
    st->phi += st->step;
    st->step += j->rate;
    if (++st->m == j->sweep) {
        st->m = 0;
        st->step = j->step0;
    }
    if (j->gate_period && ++st->g == j->gate_period)
        st->g = 0;
}

/* the jammer's contribution to the current sample, added to *ji, *jq */
GSS_JAM_HD void gss_jam_add(const gss_jam_t *j, const gss_jam_state_t *st, const uint32_t *lut,
                            int32_t *ji, int32_t *jq)
{
    if (j->gate_period && st->g >= j->gate_on)
        return;
    const uint32_t cs = lut[st->phi >> 55];
    const int32_t c = (int32_t)(int16_t)(cs & 0xFFFFu), s = (int32_t)cs >> 16;
    *ji += ((int32_t)j->amp * c + (1 << 15)) >> 16;
    *jq += ((int32_t)j->amp * s + (1 << 15)) >> 16;
}

#endif /* GSS_JAM_H */
