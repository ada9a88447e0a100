/*
 * gss_fir.hip — the front-end band-limit filter on the GPU (gss_fir_device,
 * include/gpssim_amd.h): one gfx950 kernel per output format over the SC16 samples that the
 * impairment or the jammers wrote, out of place.  It is the stages' common shape
 * (gss_stage_dev.h: groups, edges, grid), the groups taken a tile at a time:
 *
 *   samples  a tile of 256 groups per workgroup and trip; grid-stride over the tiles
 *   staging  the tile and the 64 samples before it go into LDS once, de-interleaved: one array
 *            of 32-bit words per component, a word holding two consecutive samples.  The tile
 *            itself by 16-byte loads; the 64 samples before it one per lane, from the input,
 *            the halo (the first tile of a call alone) or zeros
 *   thread   its window (32 words of history and its group's own, per component) is read from
 *            LDS into registers once; every output is a chain of packed dot products
 *            (__builtin_amdgcn_sdot2: v_dot2c_i32_i16) of window words and tap pairs
 *   taps     paired on the host for both parities of an output's distance to a word
 *            (gss_fir_pairs) and passed by value: every index into them is a constant of the
 *            unrolled loop, which leaves at a wave-uniform test on n_taps
 *   edges    an item at a time through the definition, from global memory.  An input that is
 *            not 4-byte aligned,
 *            or an input and output whose boundaries never coincide, has no whole group: the
 *            call is then all edges, at the plain form's speed (18 to 46 times slower at the
 *            headline window).  gss_run's buffers are aligned
 *   plain    GSS_FIR_PATH=plain (read per call): every output that way (gss_fir_plain_kernel)
 * The arithmetic is csrc/common/gss_fir.h, shared with the host statement gss_fir_host; sums of
 * at most 32768 * 65535 are exact in int32 in any order.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "gss_stage_dev.h"
#include "../common/gss_fir.h"

extern "C" int gss_fir_args(const gss_fir_t *fir, const void *in, const void *halo, size_t n,
                            int fmt, const void *out);                         /* fir.c */

namespace {

constexpr int FIR_THREADS = STAGE_THREADS;
constexpr int FIR_HIST = GSS_MAXTAP;            /* samples staged before a tile (>= T - 1)      */

struct FirArgs {
    const int16_t *in, *halo;
    void *out;
    uint64_t n;             /* samples                                                          */
    uint64_t head;          /* samples before the first whole group (multiple of 4 for SC01)    */
    uint64_t groups;        /* whole groups from `head` on                                      */
    int32_t n_taps;
    uint32_t even[GSS_FIR_NE], odd[GSS_FIR_NO];      /* gss_fir_pairs                           */
};

typedef short fir_s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int32_t fir_dot2(uint32_t x, uint32_t h, int32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(fir_s2, x), __builtin_bit_cast(fir_s2, h), acc,
                                  false);
#else
    return acc + (int16_t)(x & 0xFFFFu) * (int16_t)(h & 0xFFFFu) +
           (int16_t)(x >> 16) * (int16_t)(h >> 16);             /* the host pass only parses this */
#endif
}

/* one output from the definition and global memory: v (rounded) of component c of sample j.  The
   tap of index k is the low half of a pair; k is a constant in every copy of the body */
__device__ __forceinline__ void fir_sample(const FirArgs &A, uint64_t j, int32_t *vi, int32_t *vq)
{
    int32_t ai = 0, aq = 0;
#pragma unroll
    for (int k = 0; k < GSS_MAXTAP; k++) {
        if (k >= A.n_taps)
            break;
        const int32_t h = (int16_t)(((k & 1) ? A.odd[k / 2] : A.even[k / 2]) & 0xFFFFu);
        const int64_t i = (int64_t)j - k;
        ai += h * gss_fir_x(A.in, A.halo, A.n_taps, i, 0);
        aq += h * gss_fir_x(A.in, A.halo, A.n_taps, i, 1);
    }
    *vi = gss_fir_round(ai);
    *vq = gss_fir_round(aq);
}

/* one edge item: a sample (SC16, SC08) or the 4 samples of a byte (SC01) at index j */
template <int FMT> __device__ __forceinline__ void fir_item(const FirArgs &A, uint64_t j)
{
    constexpr int ITEM = StageFmt<FMT>::ITEM;
    int32_t v[2 * ITEM];
#pragma unroll
    for (int s = 0; s < ITEM; s++)
        fir_sample(A, j + s, &v[2 * s], &v[2 * s + 1]);
    stage_store_item<FMT>(A.out, j, v);
}

template <int FMT>
__global__ __launch_bounds__(FIR_THREADS) void gss_fir_kernel(FirArgs A)
{
    constexpr int NS = StageFmt<FMT>::NS, ITEM = StageFmt<FMT>::ITEM;
    constexpr int TILE = FIR_THREADS * NS;               /* samples per workgroup and trip      */
    constexpr int WORDS = (FIR_HIST + TILE) / 2;         /* per component                       */
    constexpr int WIN = FIR_HIST / 2 + NS / 2;           /* a thread's window, words            */
    __shared__ uint32_t S[2][WORDS];                     /* [component][(sample - first) / 2]   */
    const int tid = threadIdx.x;
    const uint64_t tiles = (A.groups + FIR_THREADS - 1) / FIR_THREADS;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t base = A.head + t * TILE;         /* the tile's first sample             */
        const uint64_t g = t * FIR_THREADS + tid;
        __syncthreads();                                 /* the last trip's reads are done      */
        if (tid < FIR_HIST) {                            /* sample base - 64 + tid              */
            const int64_t i = (int64_t)base - FIR_HIST + tid;
            int16_t *s16 = reinterpret_cast<int16_t *>(&S[0][0]);
            s16[tid] = (int16_t)gss_fir_x(A.in, A.halo, A.n_taps, i, 0);
            s16[2 * WORDS + tid] = (int16_t)gss_fir_x(A.in, A.halo, A.n_taps, i, 1);
        }
        if (g < A.groups) {
            const uint4 *src =
                reinterpret_cast<const uint4 *>(A.in + 2 * (base + (uint64_t)tid * NS));
#pragma unroll
            for (int u = 0; u < NS / 4; u++) {
                const uint4 r = src[u];
                const int w = FIR_HIST / 2 + tid * (NS / 2) + 2 * u;
                S[0][w] = (r.x & 0xFFFFu) | (r.y << 16);
                S[0][w + 1] = (r.z & 0xFFFFu) | (r.w << 16);
                S[1][w] = (r.x >> 16) | (r.y & 0xFFFF0000u);
                S[1][w + 1] = (r.z >> 16) | (r.w & 0xFFFF0000u);
            }
        }
        __syncthreads();
        if (g >= A.groups)
            continue;
        /* window word i holds samples n0 - 64 + 2 i and the next, n0 the group's first sample */
        uint32_t W[2][WIN];
#pragma unroll
        for (int i = 0; i < WIN; i++) {
            W[0][i] = S[0][tid * (NS / 2) + i];
            W[1][i] = S[1][tid * (NS / 2) + i];
        }
        int32_t acc[2 * NS];
#pragma unroll
        for (int i = 0; i < 2 * NS; i++)
            acc[i] = 0;
        /* output r: even r reads word r / 2 + 32 - q with even[q], q = 0..T / 2 (taps 2 q and
           2 q - 1); odd r reads word (r - 1) / 2 + 32 - q with odd[q], q = 0..(T - 1) / 2 (taps
           2 q + 1 and 2 q) */
#pragma unroll
        for (int q = 0; q < GSS_FIR_NE; q++) {
            if (2 * q > A.n_taps)
                break;
#pragma unroll
            for (int r = 0; r < NS; r += 2) {
                acc[2 * r] = fir_dot2(W[0][r / 2 + 32 - q], A.even[q], acc[2 * r]);
                acc[2 * r + 1] = fir_dot2(W[1][r / 2 + 32 - q], A.even[q], acc[2 * r + 1]);
            }
            if (q == GSS_FIR_NO)
                break;
#pragma unroll
            for (int r = 1; r < NS; r += 2) {
                acc[2 * r] = fir_dot2(W[0][r / 2 + 32 - q], A.odd[q], acc[2 * r]);
                acc[2 * r + 1] = fir_dot2(W[1][r / 2 + 32 - q], A.odd[q], acc[2 * r + 1]);
            }
        }
        int32_t v[2 * NS];
#pragma unroll
        for (int i = 0; i < 2 * NS; i++)
            v[i] = gss_fir_round(acc[i]);
        stage_store_group<FMT>(A.out, base + (uint64_t)tid * NS, v);
    }
    const uint64_t t0 = (uint64_t)blockIdx.x * FIR_THREADS + tid;
    const uint64_t stride = (uint64_t)gridDim.x * FIR_THREADS;
    for (uint64_t e = t0; e < stage_edge_items<NS, ITEM>(A.n, A.groups); e += stride)
        fir_item<FMT>(A, stage_edge_at<NS, ITEM>(e, A.head, A.groups));
}

template <int FMT>
__global__ __launch_bounds__(FIR_THREADS) void gss_fir_plain_kernel(FirArgs A)
{
    constexpr int ITEM = StageFmt<FMT>::ITEM;
    const uint64_t t0 = (uint64_t)blockIdx.x * FIR_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * FIR_THREADS;
    for (uint64_t e = t0; e < A.n / ITEM; e += stride)
        fir_item<FMT>(A, e * ITEM);
}

template <int FMT> void launch(const FirArgs &A, bool plain, unsigned grid, hipStream_t st)
{
    if (plain)
        hipLaunchKernelGGL(gss_fir_plain_kernel<FMT>, dim3(grid), dim3(FIR_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(gss_fir_kernel<FMT>, dim3(grid), dim3(FIR_THREADS), 0, st, A);
}

}  // namespace

extern "C" int gss_fir_device(gss_dev *d, const gss_fir_t *fir, const int16_t *in,
                              const int16_t *halo, size_t n, int fmt, void *out, void *stream)
{
    if (!d)
        return gss_fail(GSS_E_ARG, "invalid filter arguments");
    const int rc = gss_fir_args(fir, in, halo, n, fmt, out);
    if (rc || n == 0)
        return rc;
    const char *path = getenv("GSS_FIR_PATH");
    const bool plain = path && strcmp(path, "plain") == 0;
    if (path && *path && !plain)
        return gss_fail(GSS_E_ARG, "GSS_FIR_PATH: '%s' (plain, or unset)", path);
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    FirArgs A;
    memset(&A, 0, sizeof A);
    A.in = in; A.halo = halo; A.out = out; A.n = n; A.n_taps = fir->n_taps;
    gss_fir_pairs(fir, A.even, A.odd);
    if (!plain)                                     /* plain: head 0, no group, n / item items */
        gss_stage_split((uintptr_t)in, (uintptr_t)out, n, fmt, &A.head, &A.groups);
    const unsigned grid = gss_stage_grid(A.groups, gss_stage_items(n, A.groups, fmt), FIR_THREADS);
    stage_dispatch(fmt, [&](auto F) {
        launch<decltype(F)::value>(A, plain, grid, (hipStream_t)stream);
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "filter kernel: %s", hipGetErrorString(e));
}
