/*
 * gss_impair.h — the additive-noise impairment as host/device functions, exact integer
 * arithmetic (include/gpssim_amd.h, gss_impair_t).  The same code runs in the GPU kernels
 * (csrc/hip/gss_impair.hip) and in the host statement gss_impair_host (csrc/host/impair.c);
 * tests/test_impair.py holds an independent numpy restatement.
 *
 *   words   Philox4x32-10 (Salmon et al., SC'11) of counter {lo32(n >> 1), hi32(n >> 1), 0, 0}
 *           under key {lo32(seed), hi32(seed)}: sample n takes word 2 (n & 1) for I and the next
 *           for Q, so one call serves two samples, and a sample's noise depends on its absolute
 *           index alone
 *   normal  from one word u: sign u >> 31, cell (u >> 19) & 4095, fraction (u >> 3) & 0xFFFF of
 *           the half-normal inverse-CDF table T (Q16, 4097 entries), linearly interpolated
 *   noise   g = (mag * sigma_q8 + 2^23) >> 24, negated by the sign
 *   level   w = (x16 + g + ((1 << shift) >> 1)) >> shift (arithmetic), then the format's clamp
 */
#ifndef GSS_IMPAIR_H
#define GSS_IMPAIR_H

#include <stdint.h>
#include "gpssim_amd.h"

#if defined(__HIPCC__)
#define GSS_IMP_HD __host__ __device__ inline
#else
#define GSS_IMP_HD static inline
#endif

#define GSS_IMP_TBL 4097                 /* entries of the table: cells 0..4095 and the end */

/* Philox4x32-10 with counter words 2 and 3 zero */
GSS_IMP_HD void gss_imp_philox(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t *w)
{
    uint32_t c2 = 0, c3 = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

/* the noise of one component from its word */
GSS_IMP_HD int32_t gss_imp_noise(uint32_t u, const int32_t *T, uint32_t sigma_q8)
{
    const uint32_t idx = (u >> 19) & 4095u, f = (u >> 3) & 0xFFFFu;
    const uint32_t t0 = (uint32_t)T[idx], t1 = (uint32_t)T[idx + 1];
    const uint32_t mag = t0 + (((t1 - t0) * f) >> 16);          /* < 2^18; the product < 2^31 */
    const int32_t g = (int32_t)(((uint64_t)mag * sigma_q8 + (1u << 23)) >> 24);
    return (u >> 31) ? -g : g;
}

/* the attenuated sum, before the format's clamp */
GSS_IMP_HD int32_t gss_imp_level(int32_t x16, int32_t g, int shift)
{
    return (x16 + g + ((1 << shift) >> 1)) >> shift;
}

GSS_IMP_HD int32_t gss_imp_sc16(int32_t w) { return w < -32768 ? -32768 : w > 32767 ? 32767 : w; }
GSS_IMP_HD int32_t gss_imp_sc08(int32_t w)
{
    w >>= 4;
    return w < -128 ? -128 : w > 127 ? 127 : w;
}

#endif /* GSS_IMPAIR_H */
