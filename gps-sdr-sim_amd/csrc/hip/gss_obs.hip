/*
 * gss_obs.hip — the observables of tracked signals on the GPU (gss_obs_device, include/
 * gpssim_amd.h): per job the code phase and the accumulated carrier at the fix
 * instants, from the job's records by two int64 prefix sums modulo 2^64.
 *
 * One workgroup of four waves per job, jobs beside each other.  The workgroup walks the job's
 * records in tiles of 1,024: a lane takes four consecutive records (their s, w and dcs, and the s
 * of the record behind them for the last length), sums what they add to phi and A serially, and
 * the lanes' sums are scanned in the wave by data-parallel moves within its rows of 16 lanes
 * (row_shr 1, 2, 4, 8) and lane reads of the rows' totals across them.  Lane 0 of each wave
 * leaves the wave's total in an LDS slot, and after one barrier every lane adds the slots of the
 * waves before its own; the tile's total goes into a carry that every lane keeps in registers,
 * so it is uniform without a broadcast.  The slots are double-buffered by the tile's parity: a
 * tile costs one barrier.  A record that knows its prefixes writes the instants that lie in it
 * (gss_obs_emit): nothing but the observables is written, and no prefix goes through memory.
 * The job's last record has no successor; its length is tracking's, from its own phi.  At the
 * end the lanes mark the instants before the first record and behind the last.
 *
 * The plain form (GSS_OBS_PATH=plain) is the test partner: one lane walks a job serially
 * (gss_obs_walk, the host's statement).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "../common/gss_obs.h"

extern "C" int gss_obs_check_args(int32_t fs_hz, int64_t pitch, int n_job, int64_t t_first,
                                  int64_t step, int32_t n_fix);             /* obs.c */

namespace {

constexpr int OBS_THREADS = 256;                     /* four waves per job                      */
constexpr int OBS_WAVES = OBS_THREADS / 64;
constexpr int OBS_ITEMS = 4;                         /* consecutive records per lane            */
constexpr int OBS_TILE = OBS_THREADS * OBS_ITEMS;
constexpr int OBS_PLAIN_THREADS = 64;

struct ObsArgs {
    const gss_trk_rec_t *rec;
    const int32_t *count;
    gss_obs_t *obs;
    int64_t pitch, cs_nom, t_first, step;
    int32_t n_job, n_fix;
};

/* v plus the v of the lane CTRL names, 0 where that lane lies outside the row (the move leaves
   such a lane's destination at the old value, 0) */
template <int CTRL> __device__ __forceinline__ uint64_t dpp_add(uint64_t v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return v + ((uint64_t)(uint32_t)hi << 32 | (uint32_t)lo);
}

/* the inclusive scan of v over the wave, every lane active; *total: the wave's sum */
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, uint64_t *total)
{
    v = dpp_add<0x111>(v);                           /* row_shr:1                               */
    v = dpp_add<0x112>(v);                           /* row_shr:2                               */
    v = dpp_add<0x114>(v);                           /* row_shr:4                               */
    v = dpp_add<0x118>(v);                           /* row_shr:8                               */
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const int row = (threadIdx.x & 63) >> 4;
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {                    /* the rows' totals sit in their last lanes */
        const uint64_t t = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, 16 * r + 15) << 32 |
                           (uint32_t)__builtin_amdgcn_readlane(lo, 16 * r + 15);
        before += r < row ? t : 0;
        all += t;
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(OBS_THREADS) void gss_obs_kernel(ObsArgs A)
{
    __shared__ uint64_t slot[2][OBS_WAVES][2];
    __shared__ int32_t k_end;
    const int tid = threadIdx.x, job = blockIdx.x;
    if (job >= A.n_job)
        return;
    int64_t count = A.count[job];
    count = count < 0 ? 0 : count > A.pitch ? A.pitch : count;
    const gss_trk_rec_t *rec = A.rec + (size_t)job * A.pitch;
    gss_obs_t *obs = A.obs + (size_t)job * A.n_fix;
    if (count == 0) {                                /* uniform over the workgroup              */
        gss_obs_mark(tid, A.n_fix, OBS_THREADS, obs);
        return;
    }
    const int32_t k_first = gss_obs_kbelow(rec[0].s, A.t_first, A.step, A.n_fix);
    uint64_t cphi = 0, cA = 0;                       /* the tiles before this one               */
    int par = 0;
    for (int64_t base = 0; base < count; base += OBS_TILE, par ^= 1) {
        const int64_t e0 = base + (int64_t)tid * OBS_ITEMS;
        int64_t s[OBS_ITEMS + 1];
        int32_t w[OBS_ITEMS], dcs[OBS_ITEMS];
#pragma unroll
        for (int i = 0; i <= OBS_ITEMS; i++) {
            s[i] = 0;
            if (e0 + i < count)
                s[i] = rec[e0 + i].s;
        }
#pragma unroll
        for (int i = 0; i < OBS_ITEMS; i++) {
            w[i] = dcs[i] = 0;
            if (e0 + i < count) {
                w[i] = rec[e0 + i].w;
                dcs[i] = rec[e0 + i].dcs;
            }
        }
        uint64_t xphi[OBS_ITEMS], xA[OBS_ITEMS];     /* the lane's records before record i      */
        uint64_t tphi = 0, tA = 0;
#pragma unroll
        for (int i = 0; i < OBS_ITEMS; i++) {
            xphi[i] = tphi;
            xA[i] = tA;
            if (e0 + i + 1 < count) {                /* the last record adds to nothing         */
                uint64_t dphi, dA;
                gss_obs_delta(s[i], w[i], dcs[i], s[i + 1], A.cs_nom, &dphi, &dA);
                tphi += dphi;
                tA += dA;
            }
        }
        uint64_t wphi, wA;
        uint64_t pphi = wave_scan(tphi, &wphi) - tphi, pA = wave_scan(tA, &wA) - tA;
        if ((tid & 63) == 0) {
            slot[par][tid >> 6][0] = wphi;
            slot[par][tid >> 6][1] = wA;
        }
        __syncthreads();
        pphi += cphi;
        pA += cA;
#pragma unroll
        for (int v = 0; v < OBS_WAVES; v++) {
            const uint64_t a = slot[par][v][0], b = slot[par][v][1];
            pphi += v < (tid >> 6) ? a : 0;
            pA += v < (tid >> 6) ? b : 0;
            cphi += a;
            cA += b;
        }
#pragma unroll
        for (int i = 0; i < OBS_ITEMS; i++) {
            const int64_t e = e0 + i;
            if (e >= count)
                break;
            const uint64_t phi = pphi + xphi[i];
            const bool last = e + 1 == count;
            const int64_t end = last ? s[i] + gss_obs_last_len(phi, A.cs_nom + dcs[i]) : s[i + 1];
            const int32_t ka = gss_obs_kbelow(s[i], A.t_first, A.step, A.n_fix);
            const int32_t kb = gss_obs_kbelow(end, A.t_first, A.step, A.n_fix);
            gss_obs_emit(s[i], w[i], dcs[i], (int32_t)e, phi, pA + xA[i], A.cs_nom, A.t_first,
                         A.step, ka, kb, obs);
            if (last)
                k_end = kb;
        }
    }
    __syncthreads();
    gss_obs_mark(tid, k_first, OBS_THREADS, obs);
    gss_obs_mark(k_end + tid, A.n_fix, OBS_THREADS, obs);
}

__global__ __launch_bounds__(OBS_PLAIN_THREADS) void gss_obs_plain_kernel(ObsArgs A)
{
    const int64_t job = (int64_t)blockIdx.x * OBS_PLAIN_THREADS + threadIdx.x;
    if (job >= A.n_job)
        return;
    int64_t count = A.count[job];
    count = count < 0 ? 0 : count > A.pitch ? A.pitch : count;
    gss_obs_walk(A.rec + (size_t)job * A.pitch, (int32_t)count, A.cs_nom, A.t_first, A.step,
                 A.n_fix, A.obs + (size_t)job * A.n_fix);
}

}  // namespace

extern "C" int gss_obs_device(gss_dev *d, int32_t fs_hz, const gss_trk_rec_t *d_rec, int64_t pitch,
                              const int32_t *d_count, int n_job, int64_t t_first, int64_t step,
                              int32_t n_fix, gss_obs_t *d_obs, void *stream)
{
    int rc = gss_obs_check_args(fs_hz, pitch, n_job, t_first, step, n_fix);
    if (rc)
        return rc;
    if (!d || !d_count || (pitch > 0 && !d_rec) || (n_fix > 0 && !d_obs) ||
        ((uintptr_t)d_rec & 7) || ((uintptr_t)d_obs & 7) || ((uintptr_t)d_count & 3))
        return gss_fail(GSS_E_ARG, "invalid observables buffers");
    if (n_fix == 0)
        return 0;
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    const char *path = getenv("GSS_OBS_PATH");                 /* read per call: tests switch it */
    const bool plain = path && strcmp(path, "plain") == 0;

    ObsArgs A;
    memset(&A, 0, sizeof A);
    A.rec = d_rec; A.count = d_count; A.obs = d_obs;
    A.pitch = pitch; A.cs_nom = gss_trk_cs_nom(fs_hz); A.t_first = t_first; A.step = step;
    A.n_job = n_job; A.n_fix = n_fix;
    hipStream_t st = (hipStream_t)stream;
    if (plain)
        hipLaunchKernelGGL(gss_obs_plain_kernel,
                           dim3((unsigned)((n_job + OBS_PLAIN_THREADS - 1) / OBS_PLAIN_THREADS)),
                           dim3(OBS_PLAIN_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(gss_obs_kernel, dim3((unsigned)n_job), dim3(OBS_THREADS), 0, st, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "observables kernel: %s", hipGetErrorString(e));
}

extern "C" int gss_obs(gss_dev *d, int32_t fs_hz, const gss_trk_rec_t *rec, int64_t pitch,
                       const int32_t *count, int n_job, int64_t t_first, int64_t step,
                       int32_t n_fix, gss_obs_t *obs)
{
    int rc = gss_obs_check_args(fs_hz, pitch, n_job, t_first, step, n_fix);
    if (rc)
        return rc;
    if (!d || !count || (pitch > 0 && !rec) || (n_fix > 0 && !obs))
        return gss_fail(GSS_E_ARG, "invalid observables buffers");
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    const size_t rb = (size_t)n_job * (size_t)pitch * sizeof(gss_trk_rec_t);
    const size_t ob = (size_t)n_job * (size_t)n_fix * sizeof(gss_obs_t);
    const size_t cb = (size_t)n_job * sizeof(int32_t);
    void *dr = nullptr, *dc = nullptr, *dob = nullptr;
    if (hipMalloc(&dr, rb ? rb : 8) != hipSuccess || hipMalloc(&dc, cb) != hipSuccess ||
        hipMalloc(&dob, ob ? ob : 8) != hipSuccess)
        rc = gss_fail(GSS_E_NOMEM, "observables: out of device memory");
    else if (hipMemcpy(dc, count, cb, hipMemcpyHostToDevice) != hipSuccess)
        rc = gss_fail(GSS_E_HIP, "observables: upload failed");
    for (int j = 0; j < n_job && rc == 0; j++) {             /* only the records written       */
        const int64_t n = count[j] < 0 ? 0 : count[j] > pitch ? pitch : count[j];
        if (n > 0 && hipMemcpy((gss_trk_rec_t *)dr + (size_t)j * pitch, rec + (size_t)j * pitch,
                               (size_t)n * sizeof(gss_trk_rec_t), hipMemcpyHostToDevice) != hipSuccess)
            rc = gss_fail(GSS_E_HIP, "observables: upload failed");
    }
    if (rc == 0 &&
        (rc = gss_obs_device(d, fs_hz, (const gss_trk_rec_t *)dr, pitch, (const int32_t *)dc, n_job,
                             t_first, step, n_fix, (gss_obs_t *)dob, nullptr)) == 0 &&
        ob && hipMemcpy(obs, dob, ob, hipMemcpyDeviceToHost) != hipSuccess)
        rc = gss_fail(GSS_E_HIP, "observables: %s", hipGetErrorString(hipGetLastError()));
    (void)hipFree(dr);
    (void)hipFree(dc);
    (void)hipFree(dob);
    return rc;
}
