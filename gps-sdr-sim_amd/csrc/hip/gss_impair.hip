/*
 * gss_impair.hip — additive noise on the GPU (gss_impair_device, include/gpssim_amd.h): one
 * streaming gfx950 kernel per output format over the SC16 samples a render wrote.  It is the
 * stages' common shape (gss_stage_dev.h: groups, edges, grid, noise) with nothing between the
 * load and the noise:
 *
 *   table    the 16 KB half-normal table from LDS (each block copies it in once; the capped grid
 *            keeps that to 2,048 copies); -DGSS_IMP_TBL_L2: from global memory, a measurement
 *            build
 *   ODD      a range whose first group starts at an odd absolute index takes the ODD instance of
 *            the group for all of them (wave-uniform)
 * The arithmetic is csrc/common/gss_impair.h, shared with the host statement gss_impair_host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "gss_stage_dev.h"

extern "C" int gss_impair_check(const gss_impair_t *p, const void *iq, uint64_t sample0, size_t n,
                                int fmt, const void *out);                    /* impair.c */

namespace {

struct ImpArgs {
    const int16_t *iq;
    void *out;
    const int32_t *tbl;     /* gss_noise_table on the device (the handle's, made at open)        */
    uint64_t sample0;       /* absolute index of iq's first sample                              */
    uint64_t n;             /* samples                                                          */
    uint64_t head;          /* samples before the first whole group (multiple of 4 for SC01)    */
    uint64_t groups;        /* whole groups from `head` on                                      */
    StageNoise nz;
};

/* one group from local index j, ODD = (sample0 + j) & 1 */
template <int FMT, int ODD>
__device__ __forceinline__ void imp_group(const ImpArgs &A, const int32_t *T, uint64_t j)
{
    constexpr int NS = StageFmt<FMT>::NS;
    int4 in[NS / 4];
    int32_t v[2 * NS];
    stage_load_group<NS>(A.iq, j, in);
    stage_noise_group<NS, ODD>(A.nz, T, A.sample0 + j, [&](int i) { return stage_comp(in, i); }, v);
    stage_store_group<FMT>(A.out, j, v);
}

template <int FMT>
__global__ __launch_bounds__(STAGE_THREADS) void gss_impair_kernel(ImpArgs A)
{
    constexpr int NS = StageFmt<FMT>::NS, ITEM = StageFmt<FMT>::ITEM;
#ifdef GSS_IMP_TBL_L2                 /* measurement build: the cells from global memory (L2) */
    const int32_t *T = A.tbl;
#else
    __shared__ int32_t T[GSS_IMP_TBL];
    stage_fill_noise(T, A.tbl);
    __syncthreads();
#endif
    const uint64_t t0 = (uint64_t)blockIdx.x * STAGE_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * STAGE_THREADS;
    if ((A.sample0 + A.head) & 1) {
        for (uint64_t g = t0; g < A.groups; g += stride)
            imp_group<FMT, 1>(A, T, A.head + g * NS);
    } else {
        for (uint64_t g = t0; g < A.groups; g += stride)
            imp_group<FMT, 0>(A, T, A.head + g * NS);
    }
    for (uint64_t e = t0; e < stage_edge_items<NS, ITEM>(A.n, A.groups); e += stride) {
        const uint64_t j = stage_edge_at<NS, ITEM>(e, A.head, A.groups);
        int32_t v[2 * ITEM];
        stage_load_item<ITEM>(A.iq, j, v);
        stage_noise_item<ITEM>(A.nz, T, A.sample0 + j, v);
        stage_store_item<FMT>(A.out, j, v);
    }
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
    ImpArgs A;
    A.iq = iq; A.out = out; A.tbl = d->tab.p->noise; A.sample0 = sample0; A.n = n;
    A.nz = stage_noise_of(p);
    gss_stage_split((uintptr_t)iq, (uintptr_t)out, n, fmt, &A.head, &A.groups);
    const unsigned grid = gss_stage_grid(A.groups, gss_stage_items(n, A.groups, fmt), STAGE_THREADS);
    stage_dispatch(fmt, [&](auto F) {
        hipLaunchKernelGGL(gss_impair_kernel<decltype(F)::value>, dim3(grid), dim3(STAGE_THREADS), 0,
                           (hipStream_t)stream, A);
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "impair kernel: %s", hipGetErrorString(e));
}
