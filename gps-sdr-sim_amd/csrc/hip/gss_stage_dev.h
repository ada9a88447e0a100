/*
 * gss_stage_dev.h — the device side of the post-render stages' common shape (DESIGN.md §11.4;
 * the host side and the split rule are csrc/common/gss_stage.h).  gss_impair.hip, gss_jam.hip,
 * gss_echo.hip and gss_fir.hip are streaming gfx950 kernels of 256 threads over SC16 samples:
 *
 *   groups   a thread takes the NS samples of one wide store (StageFmt): 16-byte loads
 *            (stage_load_group), then one 16-byte store (SC16: 4 samples, SC08: 8) or one dword
 *            of bits (SC01: 16 samples, gpssim.c:2266-2276's bit order, little-endian bytes)
 *            from 2 NS int32 levels (stage_store_group)
 *   edges    the samples before the first group (where input and output are aligned to their
 *            access width) and after the last go an item at a time (a sample; SC01: a byte)
 *            through the same arithmetic (stage_edge_at, stage_load_item, stage_store_item): any
 *            n, any 2-byte aligned pointers
 *   grid     grid-stride loops under a cap of 2,048 workgroups (gss_stage_grid), which also bounds
 *            the copies of the tables the blocks make in LDS (stage_fill_noise, stage_fill_lut)
 *   noise    one Philox4x32-10 call per two samples, keyed on the absolute sample index, so a
 *            group that starts at an odd index spends one call more (the ODD instances;
 *            wave-uniform); two adjacent cells of the 16 KB half-normal table per component
 *            (stage_noise_group, stage_noise_item; the arithmetic is gss_impair.h)
 * Everything here is inlined into the kernel that calls it.
 */
#ifndef GSS_STAGE_DEV_H
#define GSS_STAGE_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "gpssim_amd.h"
#include "../common/gss_impair.h"
#include "../common/gss_jam.h"
#include "../common/gss_stage.h"

constexpr int STAGE_THREADS = 256;

template <int FMT> struct StageFmt;     /* samples of a group and of an edge item */
template <> struct StageFmt<GSS_FMT_SC16> { static constexpr int NS = 4, ITEM = 1; };
template <> struct StageFmt<GSS_FMT_SC08> { static constexpr int NS = 8, ITEM = 1; };
template <> struct StageFmt<GSS_FMT_SC01> { static constexpr int NS = 16, ITEM = 4; };

/* f(std::integral_constant<int, fmt>): the format as a compile-time constant */
template <class F> void stage_dispatch(int fmt, F f)
{
    if (fmt == GSS_FMT_SC16)
        f(std::integral_constant<int, GSS_FMT_SC16>{});
    else if (fmt == GSS_FMT_SC08)
        f(std::integral_constant<int, GSS_FMT_SC08>{});
    else
        f(std::integral_constant<int, GSS_FMT_SC01>{});
}

/* what the noise needs beside the table: gss_impair_t as the kernels take it */
struct StageNoise {
    uint32_t k0, k1, sigma_q8;
    int32_t shift;
};

inline StageNoise stage_noise_of(const gss_impair_t *p)
{
    return {(uint32_t)p->seed, (uint32_t)(p->seed >> 32), p->sigma_q8, p->shift};
}

/* the block's copy of the 16 KB noise table, and of the packed cos/sin table (cos and sin in one
   dword, 2 KB, from the handle's cos512 then sin512); __syncthreads() is the caller's */
__device__ __forceinline__ void stage_fill_noise(int32_t *T, const int32_t *tbl)
{
    for (int i = threadIdx.x; i < GSS_IMP_TBL; i += STAGE_THREADS)
        T[i] = tbl[i];
}

__device__ __forceinline__ void stage_fill_lut(uint32_t *L, const int16_t *lut)
{
    for (int i = threadIdx.x; i < GSS_JAM_LUT; i += STAGE_THREADS)
        L[i] = gss_jam_cell(lut[i], lut[GSS_JAM_LUT + i]);
}

/* the edges [0, head) and [head + groups * NS, n): their items, and the first sample of item e */
template <int NS, int ITEM>
__device__ __forceinline__ uint64_t stage_edge_items(uint64_t n, uint64_t groups)
{
    return (n - groups * NS) / ITEM;
}

template <int NS, int ITEM>
__device__ __forceinline__ uint64_t stage_edge_at(uint64_t e, uint64_t head, uint64_t groups)
{
    const uint64_t j = e * ITEM;
    return j < head ? j : j + groups * NS;
}

/* the NS samples from index j (16-byte aligned there), as loaded; stage_comp: component i of them
   (2 s for I, 2 s + 1 for Q of sample s; i a constant of an unrolled loop) */
template <int NS>
__device__ __forceinline__ void stage_load_group(const int16_t *iq, uint64_t j, int4 (&in)[NS / 4])
{
    const int4 *src = reinterpret_cast<const int4 *>(iq + 2 * j);
#pragma unroll
    for (int u = 0; u < NS / 4; u++)
        in[u] = src[u];
}

template <int NQ> __device__ __forceinline__ int32_t stage_comp(const int4 (&in)[NQ], int i)
{
    const int4 &r = in[i / 8];
    const int s = (i / 2) & 3;
    const int32_t pr = s == 0 ? r.x : s == 1 ? r.y : s == 2 ? r.z : r.w;
    return (i & 1) ? pr >> 16 : (int32_t)(int16_t)(pr & 0xFFFF);
}

template <int ITEM>
__device__ __forceinline__ void stage_load_item(const int16_t *iq, uint64_t j, int32_t (&v)[2 * ITEM])
{
#pragma unroll
    for (int i = 0; i < 2 * ITEM; i++)
        v[i] = iq[2 * j + i];
}

/* the group's 2 NS levels, clamped and packed, to `out` at sample j (aligned to the store there) */
template <int FMT>
__device__ __forceinline__ void stage_store_group(void *out, uint64_t j,
                                                  const int32_t (&v)[2 * StageFmt<FMT>::NS])
{
    if constexpr (FMT == GSS_FMT_SC16) {
        uint32_t o[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
            o[s] = ((uint32_t)gss_imp_sc16(v[2 * s]) & 0xFFFFu) |
                   ((uint32_t)gss_imp_sc16(v[2 * s + 1]) << 16);
        *reinterpret_cast<uint4 *>((int16_t *)out + 2 * j) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if constexpr (FMT == GSS_FMT_SC08) {
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            o[d] = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                o[d] |= ((uint32_t)gss_imp_sc08(v[4 * d + b]) & 0xFFu) << (8 * b);
        }
        *reinterpret_cast<uint4 *>((int8_t *)out + 2 * j) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        uint32_t o = 0;                                /* component i -> byte i / 8, bit 7 - i % 8 */
#pragma unroll
        for (int i = 0; i < 2 * StageFmt<FMT>::NS; i++)
            o |= (v[i] > 0 ? 1u : 0u) << (8 * (i / 8) + 7 - (i % 8));
        *reinterpret_cast<uint32_t *>((uint8_t *)out + j / 4) = o;
    }
}

/* one edge item's levels to `out` at sample j: a sample (SC16, SC08) or the byte of 4 (SC01) */
template <int FMT>
__device__ __forceinline__ void stage_store_item(void *out, uint64_t j,
                                                 const int32_t (&v)[2 * StageFmt<FMT>::ITEM])
{
    if constexpr (FMT == GSS_FMT_SC16) {
        ((int16_t *)out)[2 * j] = (int16_t)gss_imp_sc16(v[0]);
        ((int16_t *)out)[2 * j + 1] = (int16_t)gss_imp_sc16(v[1]);
    } else if constexpr (FMT == GSS_FMT_SC08) {
        ((int8_t *)out)[2 * j] = (int8_t)gss_imp_sc08(v[0]);
        ((int8_t *)out)[2 * j + 1] = (int8_t)gss_imp_sc08(v[1]);
    } else {
        uint32_t byte = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            byte |= (v[i] > 0 ? 1u : 0u) << (7 - i);
        ((uint8_t *)out)[j / 4] = (uint8_t)byte;
    }
}

/* the levels v of the NS samples from absolute index a: component i is x(i) plus its noise,
   attenuated.  ODD = a & 1 */
template <int NS, int ODD, class X>
__device__ __forceinline__ void stage_noise_group(const StageNoise &N, const int32_t *T, uint64_t a,
                                                  X x, int32_t (&v)[2 * NS])
{
    constexpr int NC = NS / 2 + ODD;
    uint32_t w[NC][4];
    const uint64_t c = a >> 1;
#pragma unroll
    for (int q = 0; q < NC; q++)
        gss_imp_philox((uint32_t)(c + q), (uint32_t)((c + q) >> 32), N.k0, N.k1, w[q]);
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int call = (s + ODD) >> 1, half = (s + ODD) & 1;
        v[2 * s] = gss_imp_level(x(2 * s), gss_imp_noise(w[call][2 * half], T, N.sigma_q8), N.shift);
        v[2 * s + 1] = gss_imp_level(x(2 * s + 1),
                                     gss_imp_noise(w[call][2 * half + 1], T, N.sigma_q8), N.shift);
    }
}

/* the same of an edge item's samples, each from its own call */
template <int ITEM>
__device__ __forceinline__ void stage_noise_item(const StageNoise &N, const int32_t *T, uint64_t a0,
                                                 int32_t (&v)[2 * ITEM])
{
#pragma unroll
    for (int s = 0; s < ITEM; s++) {
        const uint64_t a = a0 + s;
        uint32_t w[4];
        gss_imp_philox((uint32_t)(a >> 1), (uint32_t)(a >> 33), N.k0, N.k1, w);
        const uint32_t ui = (a & 1) ? w[2] : w[0], uq = (a & 1) ? w[3] : w[1];
        v[2 * s] = gss_imp_level(v[2 * s], gss_imp_noise(ui, T, N.sigma_q8), N.shift);
        v[2 * s + 1] = gss_imp_level(v[2 * s + 1], gss_imp_noise(uq, T, N.sigma_q8), N.shift);
    }
}

#endif /* GSS_STAGE_DEV_H */
