/*
 * gss_jam.hip — jammers beside the additive noise on the GPU (gss_jam_device,
 * include/gpssim_amd.h): one streaming gfx950 kernel per output format and per NOISE over the
 * SC16 samples a render wrote.  It is the stages' common shape (gss_stage_dev.h: groups, edges,
 * grid, noise) with the jammers' sums between the load and the noise:
 *
 *   jammers  per jammer, the state of the group's first sample from its absolute index (one
 *            64-by-32-bit division; a tone needs none), then per sample two 64-bit additions,
 *            the sweep's and the gate's counters, and one cell of the packed carrier table (2 KB
 *            of LDS); the loop over the jammers is wave-uniform.  An edge item is seeded from
 *            its own index
 *   noise    NOISE: the 16 KB table in LDS and the ODD instances, as gss_impair.hip; !NOISE
 *            (sigma_q8 == 0, where the noise is identically 0): no Philox and no table, the
 *            jammer-only path
 * The arithmetic is csrc/common/gss_jam.h and gss_impair.h, shared with gss_jam_host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "gss_stage_dev.h"

extern "C" int gss_impair_check(const gss_impair_t *p, const void *iq, uint64_t sample0, size_t n,
                                int fmt, const void *out);                    /* impair.c */
extern "C" int gss_jam_check(const gss_jam_t *jam, int n_jam);                /* jam.c */

namespace {

struct JamArgs {
    const int16_t *iq;
    void *out;
    const int32_t *tbl;     /* gss_noise_table on the device (the handle's)                     */
    const int16_t *lut;     /* cos512 then sin512 on the device (the handle's)                  */
    uint64_t sample0;       /* absolute index of iq's first sample                              */
    uint64_t n;             /* samples                                                          */
    uint64_t head;          /* samples before the first whole group (multiple of 4 for SC01)    */
    uint64_t groups;        /* whole groups from `head` on                                      */
    StageNoise nz;
    int32_t n_jam;
    gss_jam_t jam[GSS_MAXJAM];
};

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

/* the levels of samples plus jammers v without noise */
template <int NC> __device__ __forceinline__ void jam_level(const JamArgs &A, int32_t (&v)[NC])
{
#pragma unroll
    for (int i = 0; i < NC; i++)
        v[i] = gss_imp_level(v[i], 0, A.nz.shift);
}

/* one group from local index j, ODD = (sample0 + j) & 1 (NOISE only) */
template <int FMT, bool NOISE, int ODD>
__device__ __forceinline__ void jam_group(const JamArgs &A, const int32_t *T, const uint32_t *L,
                                          uint64_t j)
{
    constexpr int NS = StageFmt<FMT>::NS;
    int4 in[NS / 4];
    int32_t v[2 * NS];
    stage_load_group<NS>(A.iq, j, in);
#pragma unroll
    for (int i = 0; i < 2 * NS; i++)
        v[i] = stage_comp(in, i);
    jam_sum<NS>(A, L, A.sample0 + j, v);
    if constexpr (NOISE)
        stage_noise_group<NS, ODD>(A.nz, T, A.sample0 + j, [&](int i) { return v[i]; }, v);
    else
        jam_level(A, v);
    stage_store_group<FMT>(A.out, j, v);
}

template <int FMT, bool NOISE>
__global__ __launch_bounds__(STAGE_THREADS) void gss_jam_kernel(JamArgs A)
{
    constexpr int NS = StageFmt<FMT>::NS, ITEM = StageFmt<FMT>::ITEM;
    __shared__ uint32_t L[GSS_JAM_LUT];
    __shared__ int32_t T[NOISE ? GSS_IMP_TBL : 1];
    stage_fill_lut(L, A.lut);
    if constexpr (NOISE)
        stage_fill_noise(T, A.tbl);
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * STAGE_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * STAGE_THREADS;
    if (NOISE && ((A.sample0 + A.head) & 1)) {
        for (uint64_t g = t0; g < A.groups; g += stride)
            jam_group<FMT, NOISE, NOISE ? 1 : 0>(A, T, L, A.head + g * NS);
    } else {
        for (uint64_t g = t0; g < A.groups; g += stride)
            jam_group<FMT, NOISE, 0>(A, T, L, A.head + g * NS);
    }
    for (uint64_t e = t0; e < stage_edge_items<NS, ITEM>(A.n, A.groups); e += stride) {
        const uint64_t j = stage_edge_at<NS, ITEM>(e, A.head, A.groups);
        int32_t v[2 * ITEM];
        stage_load_item<ITEM>(A.iq, j, v);
        jam_sum<ITEM>(A, L, A.sample0 + j, v);
        if constexpr (NOISE)
            stage_noise_item<ITEM>(A.nz, T, A.sample0 + j, v);
        else
            jam_level(A, v);
        stage_store_item<FMT>(A.out, j, v);
    }
}

template <int FMT> void launch(const JamArgs &A, unsigned grid, hipStream_t st)
{
    if (A.nz.sigma_q8)
        hipLaunchKernelGGL((gss_jam_kernel<FMT, true>), dim3(grid), dim3(STAGE_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL((gss_jam_kernel<FMT, false>), dim3(grid), dim3(STAGE_THREADS), 0, st, A);
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
    JamArgs A;
    A.iq = iq; A.out = out; A.tbl = d->tab.p->noise; A.lut = d->tab.p->lut;
    A.sample0 = sample0; A.n = n;
    A.nz = stage_noise_of(p);
    A.n_jam = n_jam;
    for (int i = 0; i < GSS_MAXJAM; i++) {
        const gss_jam_t none = {0, 0, 0, 1, 0, 0, 0, 0, 0};
        A.jam[i] = i < n_jam ? jam[i] : none;
    }
    gss_stage_split((uintptr_t)iq, (uintptr_t)out, n, fmt, &A.head, &A.groups);
    const unsigned grid = gss_stage_grid(A.groups, gss_stage_items(n, A.groups, fmt), STAGE_THREADS);
    stage_dispatch(fmt, [&](auto F) { launch<decltype(F)::value>(A, grid, (hipStream_t)stream); });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "jam kernel: %s", hipGetErrorString(e));
}
