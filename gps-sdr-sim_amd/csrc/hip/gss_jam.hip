/*
 * gss_jam.hip — jammers beside the additive noise on the GPU (gss_jam_device,
 * include/gpssim_amd.h): one streaming gfx950 kernel per output format and per NOISE over the
 * SC16 samples a render wrote.  It has the shape of gss_impair.hip's kernel:
 *
 *   input    16-byte loads: 4 samples (I, Q int16) each
 *   jammers  per jammer, the state of the group's first sample from its absolute index (one
 *            64-by-32-bit division; a tone needs none), then per sample two 64-bit additions,
 *            the sweep's and the gate's counters, and one cell of the packed carrier table (cos
 *            and sin in one dword, 2 KB of LDS, built by each block from the handle's tables);
 *            the loop over the jammers is wave-uniform
 *   noise    NOISE: as gss_impair.hip (one Philox4x32-10 call per two samples, the 16 KB table
 *            in LDS, the ODD instances); !NOISE (sigma_q8 == 0, where the noise is identically
 *            0): no Philox and no table, the jammer-only path
 *   output   SC16: 4 samples per thread, one 16-byte store; SC08: 8 samples, one 16-byte store;
 *            SC01: 16 samples, one dword
 *   edges    the samples before the first 16-byte boundary and after the last whole group go one
 *            item at a time through the same arithmetic, each seeded from its own index
 * The arithmetic is csrc/common/gss_jam.h and gss_impair.h, shared with gss_jam_host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "../common/gss_impair.h"
#include "../common/gss_jam.h"

extern "C" int gss_impair_check(const gss_impair_t *p, const void *iq, uint64_t sample0, size_t n,
                                int fmt, const void *out);                    /* impair.c */
extern "C" int gss_jam_check(const gss_jam_t *jam, int n_jam);                /* jam.c */

namespace {

constexpr int JAM_THREADS = 256;
constexpr int JAM_GRID_MAX = 2048;

struct JamArgs {
    const int16_t *iq;
    void *out;
    const int32_t *tbl;     /* gss_noise_table on the device (the handle's)                     */
    const int16_t *lut;     /* cos512 then sin512 on the device (the handle's)                  */
    uint64_t sample0;       /* absolute index of iq's first sample                              */
    uint64_t n;             /* samples                                                          */
    uint64_t head;          /* samples before the first whole group (multiple of 4 for SC01)    */
    uint64_t groups;        /* whole groups of 4 U samples from `head` on                       */
    uint32_t k0, k1, sigma_q8;
    int32_t shift;
    int32_t n_jam;
    gss_jam_t jam[GSS_MAXJAM];
};

template <int FMT> struct JamFmt;
template <> struct JamFmt<GSS_FMT_SC16> { static constexpr int U = 1, ITEM = 1; };
template <> struct JamFmt<GSS_FMT_SC08> { static constexpr int U = 2, ITEM = 1; };
template <> struct JamFmt<GSS_FMT_SC01> { static constexpr int U = 4, ITEM = 4; };

/* the jammers' sums over NS consecutive samples from absolute index a, added to v[2 s], v[2 s + 1];
   the jammer index is a constant in every copy of the body, so the arguments stay in SGPRs */
template <int NS>
__device__ __forceinline__ void jam_sum(const JamArgs &A, const uint32_t *L, uint64_t a, int32_t *v)
{
#pragma unroll
    for (int q = 0; q < GSS_MAXJAM; q++) {
        if (q >= A.n_jam)
            break;
        const gss_jam_t jm = A.jam[q];
        gss_jam_state_t st;
        gss_jam_seed(&jm, a, &st);
#pragma unroll
        for (int s = 0; s < NS; s++) {
            gss_jam_add(&jm, &st, L, &v[2 * s], &v[2 * s + 1]);
            if (s + 1 < NS)
                gss_jam_next(&jm, &st);
        }
    }
}

/* one group: 4 U samples from local index j (input 16-byte aligned there), absolute index a;
   ODD = a & 1 (NOISE only) */
template <int FMT, bool NOISE, int ODD>
__device__ __forceinline__ void jam_group(const JamArgs &A, const int32_t *T, const uint32_t *L,
                                          uint64_t j)
{
    constexpr int U = JamFmt<FMT>::U, NS = 4 * U, NC = 2 * U + ODD;
    const uint64_t a = A.sample0 + j;
    const int4 *src = reinterpret_cast<const int4 *>(A.iq + 2 * j);
    int32_t v[2 * NS];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int4 r = src[u];
        const int32_t pr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int s = 0; s < 4; s++) {
            v[8 * u + 2 * s] = (int32_t)(int16_t)(pr[s] & 0xFFFF);
            v[8 * u + 2 * s + 1] = pr[s] >> 16;
        }
    }
    jam_sum<NS>(A, L, a, v);
    if constexpr (NOISE) {
        const uint64_t c = a >> 1;
#pragma unroll
        for (int q = 0; q < NC; q++) {
            uint32_t w[4];
            gss_imp_philox((uint32_t)(c + q), (uint32_t)((c + q) >> 32), A.k0, A.k1, w);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int s = 2 * q + h - ODD;           /* the sample that takes this half */
                if (s < 0 || s >= NS)
                    continue;
                v[2 * s] = gss_imp_level(v[2 * s], gss_imp_noise(w[2 * h], T, A.sigma_q8), A.shift);
                v[2 * s + 1] = gss_imp_level(v[2 * s + 1],
                                             gss_imp_noise(w[2 * h + 1], T, A.sigma_q8), A.shift);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2 * NS; i++)
            v[i] = gss_imp_level(v[i], 0, A.shift);
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
template <int FMT, bool NOISE>
__device__ __forceinline__ void jam_item(const JamArgs &A, const int32_t *T, const uint32_t *L,
                                         uint64_t j)
{
    constexpr int ITEM = JamFmt<FMT>::ITEM;
    int32_t v[2 * ITEM];
#pragma unroll
    for (int s = 0; s < ITEM; s++) {
        v[2 * s] = A.iq[2 * (j + s)];
        v[2 * s + 1] = A.iq[2 * (j + s) + 1];
    }
    jam_sum<ITEM>(A, L, A.sample0 + j, v);
    uint32_t byte = 0;
#pragma unroll
    for (int s = 0; s < ITEM; s++) {
        int32_t gi = 0, gq = 0;
        if constexpr (NOISE) {
            const uint64_t a = A.sample0 + j + s;
            uint32_t w[4];
            gss_imp_philox((uint32_t)(a >> 1), (uint32_t)(a >> 33), A.k0, A.k1, w);
            gi = gss_imp_noise((a & 1) ? w[2] : w[0], T, A.sigma_q8);
            gq = gss_imp_noise((a & 1) ? w[3] : w[1], T, A.sigma_q8);
        }
        const int32_t vi = gss_imp_level(v[2 * s], gi, A.shift);
        const int32_t vq = gss_imp_level(v[2 * s + 1], gq, A.shift);
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

template <int FMT, bool NOISE>
__global__ __launch_bounds__(JAM_THREADS) void gss_jam_kernel(JamArgs A)
{
    constexpr int NS = 4 * JamFmt<FMT>::U, ITEM = JamFmt<FMT>::ITEM;
    __shared__ uint32_t L[GSS_JAM_LUT];
    __shared__ int32_t T[NOISE ? GSS_IMP_TBL : 1];
    for (int i = threadIdx.x; i < GSS_JAM_LUT; i += JAM_THREADS)
        L[i] = gss_jam_cell(A.lut[i], A.lut[GSS_JAM_LUT + i]);
    if constexpr (NOISE)
        for (int i = threadIdx.x; i < GSS_IMP_TBL; i += JAM_THREADS)
            T[i] = A.tbl[i];
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * JAM_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * JAM_THREADS;
    if (NOISE && ((A.sample0 + A.head) & 1)) {
        for (uint64_t g = t0; g < A.groups; g += stride)
            jam_group<FMT, NOISE, NOISE ? 1 : 0>(A, T, L, A.head + g * NS);
    } else {
        for (uint64_t g = t0; g < A.groups; g += stride)
            jam_group<FMT, NOISE, 0>(A, T, L, A.head + g * NS);
    }
    /* the edges: [0, head) and [head + groups * NS, n) */
    const uint64_t body = A.groups * NS, items = (A.n - body) / ITEM;
    for (uint64_t e = t0; e < items; e += stride) {
        const uint64_t j = e * ITEM;
        jam_item<FMT, NOISE>(A, T, L, j < A.head ? j : j + body);
    }
}

template <int FMT> void launch(const JamArgs &A, unsigned grid, hipStream_t st)
{
    if (A.sigma_q8)
        hipLaunchKernelGGL((gss_jam_kernel<FMT, true>), dim3(grid), dim3(JAM_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL((gss_jam_kernel<FMT, false>), dim3(grid), dim3(JAM_THREADS), 0, st, A);
}

}  // namespace

extern "C" int gss_jam_device(gss_dev *d, const gss_impair_t *p, const gss_jam_t *jam, int n_jam,
                              const int16_t *iq, uint64_t sample0, size_t n, int fmt, void *out,
                              void *stream)
{
    if (!d)
        return gss_fail(GSS_E_ARG, "invalid jammer arguments");
    int rc = gss_impair_check(p, iq, sample0, n, fmt, out);
    if (!rc)
        rc = gss_jam_check(jam, n_jam);
    if (rc || n == 0)
        return rc;
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    const int U = fmt == GSS_FMT_SC16 ? 1 : fmt == GSS_FMT_SC08 ? 2 : 4;
    const int item = fmt == GSS_FMT_SC01 ? 4 : 1;
    const size_t ns = (size_t)4 * U;
    JamArgs A;
    A.iq = iq; A.out = out; A.tbl = d->tab.p->noise; A.lut = d->tab.p->lut;
    A.sample0 = sample0; A.n = n;
    A.k0 = (uint32_t)p->seed; A.k1 = (uint32_t)(p->seed >> 32);
    A.sigma_q8 = p->sigma_q8; A.shift = p->shift;
    A.n_jam = n_jam;
    for (int i = 0; i < GSS_MAXJAM; i++) {
        const gss_jam_t none = {0, 0, 0, 1, 0, 0, 0, 0, 0};
        A.jam[i] = i < n_jam ? jam[i] : none;
    }
    /* the least head after which the input is 16-byte aligned and the output aligned to its
       store (16, 16, 4 bytes); none (pointers that never line up): every sample by the edges */
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
    uint64_t grid = (work + JAM_THREADS - 1) / JAM_THREADS;
    grid = grid < 1 ? 1 : grid > JAM_GRID_MAX ? JAM_GRID_MAX : grid;
    hipStream_t st = (hipStream_t)stream;
    if (fmt == GSS_FMT_SC16)
        launch<GSS_FMT_SC16>(A, (unsigned)grid, st);
    else if (fmt == GSS_FMT_SC08)
        launch<GSS_FMT_SC08>(A, (unsigned)grid, st);
    else
        launch<GSS_FMT_SC01>(A, (unsigned)grid, st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "jam kernel: %s", hipGetErrorString(e));
}
