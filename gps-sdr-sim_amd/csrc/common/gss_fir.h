/*
 * gss_fir.h — the front-end band-limit filter as host/device functions, exact integer arithmetic
 * (include/gpssim_amd.h, gss_fir_t).  The same code runs in the GPU kernels
 * (csrc/hip/gss_fir.hip) and in the host statement gss_fir_host (csrc/host/fir.c);
 * tests/fir_oracle.py holds an independent numpy restatement.
 *
 *   sum     acc[n] = sum_{k < T} taps[k] * x_c[n - k] per component c, int32: exact in any order,
 *           since sum |taps| <= 65535 bounds |acc| by 32768 * 65535 < 2^31
 *   round   v = (acc + 2^13) >> 14 (arithmetic; acc + 2^13 < 2^31 by the same bound)
 *   output  the impairment's stage (gss_impair.h) with w = v
 *   halo    x[i] for i < 0 is halo[T - 1 + i], or 0 without a halo
 *   pairs   what the packed dot products of the kernel read: a 32-bit word holds two consecutive
 *           samples of one component (the earlier one low), and for an output at an even
 *           distance 2 q from the word's first sample the taps (taps[2 q], taps[2 q - 1]), at an
 *           odd distance 2 q + 1 the taps (taps[2 q + 1], taps[2 q]); taps outside 0..T-1 are 0
 */
#ifndef GSS_FIR_H
#define GSS_FIR_H

#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_impair.h"

#if defined(__HIPCC__)
#define GSS_FIR_HD __host__ __device__ inline
#else
#define GSS_FIR_HD static inline
#endif

#define GSS_FIR_L1_MAX 65535            /* sum |taps|                                            */
#define GSS_FIR_NE (GSS_MAXTAP / 2 + 1) /* pairs for an even distance: q = 0..32                 */
#define GSS_FIR_NO (GSS_MAXTAP / 2)     /* pairs for an odd distance:  q = 0..31                 */

/* 0 for a filter the calls accept */
GSS_FIR_HD int gss_fir_invalid(const gss_fir_t *f)
{
    if (f->n_taps < 1 || f->n_taps > GSS_MAXTAP || f->pad != 0)
        return 1;
    int32_t l1 = 0;
    for (int k = 0; k < f->n_taps; k++)
        l1 += f->taps[k] < 0 ? -(int32_t)f->taps[k] : (int32_t)f->taps[k];
    return l1 > GSS_FIR_L1_MAX;
}

GSS_FIR_HD int32_t gss_fir_round(int32_t acc) { return (acc + (1 << 13)) >> 14; }

/* component c of sample i of the call: the input, the halo before it, zeros before that */
GSS_FIR_HD int32_t gss_fir_x(const int16_t *in, const int16_t *halo, int T, int64_t i, int c)
{
    if (i >= 0)
        return in[2 * i + c];
    const int64_t h = (int64_t)(T - 1) + i;
    return halo && h >= 0 ? halo[2 * h + c] : 0;
}

/* the tap pairs of a filter: even[GSS_FIR_NE], odd[GSS_FIR_NO], low half first */
GSS_FIR_HD void gss_fir_pairs(const gss_fir_t *f, uint32_t *even, uint32_t *odd)
{
    int16_t h[GSS_MAXTAP + 2];                           /* h[1 + k] = taps[k], 0 around them    */
    for (int k = 0; k < GSS_MAXTAP + 2; k++)
        h[k] = k >= 1 && k <= f->n_taps ? f->taps[k - 1] : (int16_t)0;
    for (int q = 0; q < GSS_FIR_NE; q++)
        even[q] = (uint32_t)(uint16_t)h[1 + 2 * q] | (uint32_t)(uint16_t)h[2 * q] << 16;
    for (int q = 0; q < GSS_FIR_NO; q++)
        odd[q] = (uint32_t)(uint16_t)h[2 + 2 * q] | (uint32_t)(uint16_t)h[1 + 2 * q] << 16;
}

#endif /* GSS_FIR_H */
