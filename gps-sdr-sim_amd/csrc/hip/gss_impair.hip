/*
 * gss_impair.hip — additive noise on the GPU (gss_impair_device, include/gpssim_amd.h): one
 * streaming gfx950 kernel per output format over the SC16 samples a render wrote.
 *
 *   input    16-byte loads: 4 samples (I, Q int16) each
 *   words    one Philox4x32-10 call per two samples, keyed on the absolute sample index, so a
 *            range that starts at an odd index spends one call more per thread (the ODD
 *            instances; wave-uniform)
 *   normal   two adjacent cells of the 16 KB half-normal table per component, from LDS (each
 *            block copies the table in once; a capped grid keeps that to 2,048 copies)
 *   output   SC16: 4 samples per thread, one 16-byte store; SC08: 8 samples, one 16-byte store;
 *            SC01: 16 samples, one dword (gpssim.c:2266-2276's bit order, little-endian bytes)
 *   edges    the samples before the first 16-byte boundary of the input (and of the output's
 *            store width) and after the last whole group go one by one (SC01: byte by byte)
 *            through the same arithmetic: any sample0, any n, any 2-byte aligned pointers
 * The arithmetic is csrc/common/gss_impair.h, shared with the host statement gss_impair_host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "../common/gss_impair.h"

extern "C" int gss_impair_check(const gss_impair_t *p, const void *iq, uint64_t sample0, size_t n,
                                int fmt, const void *out);                    /* impair.c */

namespace {

constexpr int IMP_THREADS = 256;
constexpr int IMP_GRID_MAX = 2048;

struct ImpArgs {
    const int16_t *iq;
    void *out;
    const int32_t *tbl;     /* gss_noise_table on the device (the handle's, made at open)        */
    uint64_t sample0;       /* absolute index of iq's first sample                              */
    uint64_t n;             /* samples                                                          */
    uint64_t head;          /* samples before the first whole group (multiple of 4 for SC01)    */
    uint64_t groups;        /* whole groups of 4 U samples from `head` on                       */
    uint32_t k0, k1, sigma_q8;
    int32_t shift;
};

template <int FMT> struct ImpFmt;
template <> struct ImpFmt<GSS_FMT_SC16> { static constexpr int U = 1, ITEM = 1; };
template <> struct ImpFmt<GSS_FMT_SC08> { static constexpr int U = 2, ITEM = 1; };
template <> struct ImpFmt<GSS_FMT_SC01> { static constexpr int U = 4, ITEM = 4; };

/* one group: 4 U samples from local index j (input 16-byte aligned there), absolute index a;
   ODD = a & 1 */
template <int FMT, int ODD>
__device__ __forceinline__ void imp_group(const ImpArgs &A, const int32_t *T, uint64_t j)
{
    constexpr int U = ImpFmt<FMT>::U, NS = 4 * U, NC = 2 * U + ODD;
    const uint64_t a = A.sample0 + j;
    const int4 *src = reinterpret_cast<const int4 *>(A.iq + 2 * j);
    int4 in[U];
#pragma unroll
    for (int u = 0; u < U; u++)
        in[u] = src[u];
    uint32_t w[NC][4];
    const uint64_t c = a >> 1;
#pragma unroll
    for (int q = 0; q < NC; q++)
        gss_imp_philox((uint32_t)(c + q), (uint32_t)((c + q) >> 32), A.k0, A.k1, w[q]);
    int32_t v[2 * NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int4 &r = in[s / 4];
        const int32_t pr = (s & 3) == 0 ? r.x : (s & 3) == 1 ? r.y : (s & 3) == 2 ? r.z : r.w;
        const int32_t xi = (int32_t)(int16_t)(pr & 0xFFFF), xq = pr >> 16;
        const int call = (s + ODD) >> 1, half = (s + ODD) & 1;
        v[2 * s] = gss_imp_level(xi, gss_imp_noise(w[call][2 * half], T, A.sigma_q8), A.shift);
        v[2 * s + 1] = gss_imp_level(xq, gss_imp_noise(w[call][2 * half + 1], T, A.sigma_q8),
                                     A.shift);
    }
    if constexpr (FMT == GSS_FMT_SC16) {
        uint32_t o[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
            o[s] = ((uint32_t)gss_imp_sc16(v[2 * s]) & 0xFFFFu) |
                   ((uint32_t)gss_imp_sc16(v[2 * s + 1]) << 16);
        *reinterpret_cast<uint4 *>((int16_t *)A.out + 2 * j) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if constexpr (FMT == GSS_FMT_SC08) {
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            o[d] = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                o[d] |= ((uint32_t)gss_imp_sc08(v[4 * d + b]) & 0xFFu) << (8 * b);
        }
        *reinterpret_cast<uint4 *>((int8_t *)A.out + 2 * j) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        uint32_t o = 0;                                /* component i -> byte i / 8, bit 7 - i % 8 */
#pragma unroll
        for (int i = 0; i < 2 * NS; i++)
            o |= (v[i] > 0 ? 1u : 0u) << (8 * (i / 8) + 7 - (i % 8));
        *reinterpret_cast<uint32_t *>((uint8_t *)A.out + j / 4) = o;
    }
}

/* one edge item: a sample (SC16, SC08) or the 4 samples of a byte (SC01) at local index j */
template <int FMT>
__device__ __forceinline__ void imp_item(const ImpArgs &A, const int32_t *T, uint64_t j)
{
    uint32_t byte = 0;
#pragma unroll
    for (int s = 0; s < ImpFmt<FMT>::ITEM; s++) {
        const uint64_t a = A.sample0 + j + s;
        uint32_t w[4];
        gss_imp_philox((uint32_t)(a >> 1), (uint32_t)(a >> 33), A.k0, A.k1, w);
        const uint32_t ui = (a & 1) ? w[2] : w[0], uq = (a & 1) ? w[3] : w[1];
        const int32_t vi = gss_imp_level(A.iq[2 * (j + s)], gss_imp_noise(ui, T, A.sigma_q8),
                                         A.shift);
        const int32_t vq = gss_imp_level(A.iq[2 * (j + s) + 1], gss_imp_noise(uq, T, A.sigma_q8),
                                         A.shift);
        if constexpr (FMT == GSS_FMT_SC16) {
            ((int16_t *)A.out)[2 * j] = (int16_t)gss_imp_sc16(vi);
            ((int16_t *)A.out)[2 * j + 1] = (int16_t)gss_imp_sc16(vq);
        } else if constexpr (FMT == GSS_FMT_SC08) {
            ((int8_t *)A.out)[2 * j] = (int8_t)gss_imp_sc08(vi);
            ((int8_t *)A.out)[2 * j + 1] = (int8_t)gss_imp_sc08(vq);
        } else {
            byte |= (vi > 0 ? 1u : 0u) << (7 - 2 * s) | (vq > 0 ? 1u : 0u) << (6 - 2 * s);
        }
    }
    if constexpr (FMT == GSS_FMT_SC01)
        ((uint8_t *)A.out)[j / 4] = (uint8_t)byte;
}

template <int FMT>
__global__ __launch_bounds__(IMP_THREADS) void gss_impair_kernel(ImpArgs A)
{
    constexpr int NS = 4 * ImpFmt<FMT>::U, ITEM = ImpFmt<FMT>::ITEM;
#ifdef GSS_IMP_TBL_L2                 /* measurement build: the cells from global memory (L2) */
    const int32_t *T = A.tbl;
#else
    __shared__ int32_t T[GSS_IMP_TBL];
    for (int i = threadIdx.x; i < GSS_IMP_TBL; i += IMP_THREADS)
        T[i] = A.tbl[i];
    __syncthreads();
#endif
    const uint64_t t0 = (uint64_t)blockIdx.x * IMP_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * IMP_THREADS;
    if ((A.sample0 + A.head) & 1) {
        for (uint64_t g = t0; g < A.groups; g += stride)
            imp_group<FMT, 1>(A, T, A.head + g * NS);
    } else {
        for (uint64_t g = t0; g < A.groups; g += stride)
            imp_group<FMT, 0>(A, T, A.head + g * NS);
    }
    /* the edges: [0, head) and [head + groups * NS, n) */
    const uint64_t body = A.groups * NS, items = (A.n - body) / ITEM;
    for (uint64_t e = t0; e < items; e += stride) {
        const uint64_t j = e * ITEM;
        imp_item<FMT>(A, T, j < A.head ? j : j + body);
    }
}

template <int FMT> void launch(const ImpArgs &A, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL(gss_impair_kernel<FMT>, dim3(grid), dim3(IMP_THREADS), 0, st, A);
}

}  // namespace

extern "C" int gss_impair_device(gss_dev *d, const gss_impair_t *p, const int16_t *iq,
                                 uint64_t sample0, size_t n, int fmt, void *out, void *stream)
{
    if (!d)
        return gss_fail(GSS_E_ARG, "invalid impairment arguments");
    int rc = gss_impair_check(p, iq, sample0, n, fmt, out);
    if (rc || n == 0)
        return rc;
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    const int U = fmt == GSS_FMT_SC16 ? 1 : fmt == GSS_FMT_SC08 ? 2 : 4;
    const int item = fmt == GSS_FMT_SC01 ? 4 : 1;
    const size_t ns = (size_t)4 * U;
    /* the least head after which the input is 16-byte aligned and the output aligned to its
       store (16, 16, 4 bytes); none (pointers that never line up): every sample by the edges */
    ImpArgs A;
    A.iq = iq; A.out = out; A.tbl = d->tab.p->noise; A.sample0 = sample0; A.n = n;
    A.k0 = (uint32_t)p->seed; A.k1 = (uint32_t)(p->seed >> 32);
    A.sigma_q8 = p->sigma_q8; A.shift = p->shift;
    A.head = n;
    A.groups = 0;
    for (size_t h = 0; h < 16 && h <= n; h += (size_t)item) {
        const uintptr_t ai = (uintptr_t)iq + 4 * h;
        const uintptr_t ao = (uintptr_t)out + (fmt == GSS_FMT_SC16 ? 4 * h : fmt == GSS_FMT_SC08 ? 2 * h : h / 4);
        if (ai % 16 == 0 && ao % (fmt == GSS_FMT_SC01 ? 4 : 16) == 0) {
            A.head = h;
            A.groups = (n - h) / ns;
            break;
        }
    }
    const uint64_t items = (n - A.groups * ns) / (uint64_t)item;
    const uint64_t work = A.groups > items ? A.groups : items;
    uint64_t grid = (work + IMP_THREADS - 1) / IMP_THREADS;
    grid = grid < 1 ? 1 : grid > IMP_GRID_MAX ? IMP_GRID_MAX : grid;
    hipStream_t st = (hipStream_t)stream;
    if (fmt == GSS_FMT_SC16)
        launch<GSS_FMT_SC16>(A, (unsigned)grid, st);
    else if (fmt == GSS_FMT_SC08)
        launch<GSS_FMT_SC08>(A, (unsigned)grid, st);
    else
        launch<GSS_FMT_SC01>(A, (unsigned)grid, st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "impair kernel: %s", hipGetErrorString(e));
}
