/*
 * gss_track.hip — signal tracking on the GPU (gss_track_device, include/gpssim_amd.h; DESIGN.md
 * §13): per job the code and carrier loops of one satellite over the samples, one record per
 * code period.
 *
 * The loops feed back every code period, so only the samples of one epoch run in parallel and
 * the jobs beside each other: one workgroup of eight waves per job, one kernel per sample format
 * (the unpacking folds to straight code).  The carrier tables (cos and sin packed into one dword)
 * and the job's C/A row sit in LDS.  A lane takes every 512th sample of the epoch; its code and
 * carrier phases advance by additions, and its six partial sums stay in int32 registers for at
 * most 127 samples (|y| <= 16384000, 127 |y| < 2^31) before they are added to the int64 ones.
 * No sample costs a branch: a lane past the epoch's end correlates a zero sample, with its chip
 * indices masked into the LDS row.  A wave sums by data-parallel moves within its rows of 16
 * lanes and lane reads across them, lane 0 of each wave leaves the sums in an LDS slot, and after
 * one barrier every lane adds the waves' slots and computes the update (gss_trk_update) itself:
 * the state is uniform without a broadcast.  The slots are double-buffered by the epoch's
 * parity, so an epoch costs one barrier.  The next epoch starts at sample s + n, known before the
 * reduction: each lane's first six samples of it (3,072 per workgroup) are loaded ahead of the
 * barrier and kept in registers; an index past the N samples is clamped to the last one and its
 * value discarded.  Beyond those, a pass loads four samples per lane before it correlates them.
 *
 * A launch advances a job by at most `chunk` epochs (4096) and leaves its state in device
 * memory; gss_track_device loops launches, so no launch runs longer than tens of milliseconds.
 *
 * The plain form (GSS_TRK_PATH=plain) is the test partner: one wave per job, every lane sums in
 * int64 from memory, and the wave reduces through LDS alone.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "../common/gss_trk.h"

extern "C" int gss_trk_check_args(const gss_trk_cfg_t *cfg, int64_t N, const gss_trk_job_t *jobs,
                                  int n_job, int64_t pitch);                /* track.c */

namespace {

constexpr int TRK_THREADS = 512;                     /* the fast form: eight waves per job      */
constexpr int TRK_PLAIN_THREADS = 64;
constexpr int TRK_AHEAD = 3072;                      /* samples of an epoch loaded ahead        */
constexpr int TRK_FLUSH = 127;                       /* samples an int32 partial sum may hold   */
constexpr int TRK_CHUNK = 4096;                      /* epochs per launch                       */

struct TrkArgs {
    const void *x;
    const gss_trk_job_t *jobs;
    gss_trk_state_t *state;
    gss_trk_rec_t *rec;
    int32_t *count;
    const uint32_t *ca;          /* gss_ca_table                                                */
    const int16_t *lut;          /* cos512 then sin512                                          */
    int64_t N, pitch, cs_nom;
    gss_trk_cfg_t cfg;
    int32_t n_job, chunk;
    int32_t first, pad;          /* the call's first launch: the state starts from the job      */
};

struct Tables {
    uint32_t lut[512];           /* cos in the low half, sin in the high half                   */
    uint32_t ca[GSS_CA_WORDS];
};

__device__ __forceinline__ void load_tables(Tables &t, const TrkArgs &A, int prn, int nthreads)
{
    for (int i = threadIdx.x; i < 512; i += nthreads)
        t.lut[i] = (uint32_t)(uint16_t)A.lut[i] | (uint32_t)(uint16_t)A.lut[512 + i] << 16;
    for (int i = threadIdx.x; i < GSS_CA_WORDS; i += nthreads)
        t.ca[i] = A.ca[(prn - 1) * GSS_CA_WORDS + i];
}

/* the six products of one sample at code phase c and carrier phase th */
template <class Acc>
__device__ __forceinline__ void correlate(const Tables &t, int32_t xi, int32_t xq, int64_t c,
                                          uint32_t th, Acc *q)
{
    const uint32_t cs = t.lut[th >> 23];
    const int32_t co = (int16_t)(cs & 0xFFFFu), si = (int16_t)(cs >> 16);
    const int32_t yi = xi * co + xq * si, yq = xq * co - xi * si;
    const bool e = gss_acq_replica(t.ca, gss_trk_chip_early(c)) > 0;
    const bool p = gss_acq_replica(t.ca, (int32_t)(c >> 32)) > 0;
    const bool l = gss_acq_replica(t.ca, gss_trk_chip_late(c)) > 0;
    q[0] += e ? yi : -yi; q[1] += e ? yq : -yq;
    q[2] += p ? yi : -yi; q[3] += p ? yq : -yq;
    q[4] += l ? yi : -yi; q[5] += l ? yq : -yq;
}

/* The same without a branch for a lane that may be past the epoch's end: there the caller passes
   zero samples, and the chip indices are masked into the LDS row (an index below 1023 is
   unchanged; bit 1023 of the row is never set and meets a zero sample). */
__device__ __forceinline__ void correlate_any(const Tables &t, int32_t xi, int32_t xq, int64_t c,
                                              uint32_t th, int32_t *q)
{
    const uint32_t cs = t.lut[th >> 23];
    const int32_t co = (int16_t)(cs & 0xFFFFu), si = (int16_t)(cs >> 16);
    const int32_t yi = xi * co + xq * si, yq = xq * co - xi * si;
    const int64_t ce = c + GSS_TRK_HALF, cl = c - GSS_TRK_HALF;
    const uint32_t ie = (uint32_t)((ce >= GSS_TRK_M ? ce - GSS_TRK_M : ce) >> 32) & 1023u;
    const uint32_t ip = (uint32_t)(c >> 32) & 1023u;
    const uint32_t il = (uint32_t)((cl < 0 ? cl + GSS_TRK_M : cl) >> 32) & 1023u;
    const bool e = t.ca[ie >> 5] >> (ie & 31) & 1u;
    const bool p = t.ca[ip >> 5] >> (ip & 31) & 1u;
    const bool l = t.ca[il >> 5] >> (il & 31) & 1u;
    q[0] += e ? yi : -yi; q[1] += e ? yq : -yq;
    q[2] += p ? yi : -yi; q[3] += p ? yq : -yq;
    q[4] += l ? yi : -yi; q[5] += l ? yq : -yq;
}

/* sample g, or the last sample when g is past the end (the caller discards it) */
__device__ __forceinline__ void sample_clamped(const TrkArgs &A, int fmt, int64_t g, int32_t *xi,
                                               int32_t *xq)
{
    gss_acq_sample(A.x, fmt, g < A.N ? g : A.N - 1, xi, xq);
}

/* The wave's sum in every lane, every lane active.  Within a row of 16 lanes by data-parallel
   moves (lane ^ 1, lane ^ 2, the mirrored half row, the mirrored row), then the four rows' sums
   by lane reads. */
template <int CTRL> __device__ __forceinline__ int64_t dpp_add(int64_t v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(uint64_t)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), CTRL, 0xF, 0xF,
                                               false);
    return v + (int64_t)((uint64_t)(uint32_t)hi << 32 | (uint32_t)lo);
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
    v = dpp_add<0xB1>(v);                            /* quad_perm [1, 0, 3, 2]                  */
    v = dpp_add<0x4E>(v);                            /* quad_perm [2, 3, 0, 1]                  */
    v = dpp_add<0x141>(v);                           /* row_half_mirror                         */
    v = dpp_add<0x140>(v);                           /* row_mirror                              */
    const int lo = (int)(uint32_t)(uint64_t)v, hi = (int)(uint32_t)((uint64_t)v >> 32);
    int64_t r = 0;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        r += (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, l) << 32 |
                       (uint32_t)__builtin_amdgcn_readlane(lo, l));
    return r;
}

/* FMT: the sample format as a constant (the unpacking folds), or 0 for the launch's cfg.fmt */
template <bool PLAIN, int NT, int FMT>
__global__ __launch_bounds__(NT) void gss_track_kernel(TrkArgs A)
{
    constexpr int TRK_WAVES = NT / 64;
    constexpr int TRK_PF = TRK_AHEAD / NT;           /* samples per lane loaded ahead           */
    constexpr int TRK_U = 4;                         /* samples per lane and loop pass beyond   */
    static_assert(TRK_PF >= 1 && TRK_PF + TRK_U <= TRK_FLUSH, "an int32 sum holds a pass");
    __shared__ Tables tab;
    __shared__ int64_t slot[PLAIN ? 1 : 2][PLAIN ? NT : TRK_WAVES][6];
    const int tid = threadIdx.x, job = blockIdx.x;
    if (job >= A.n_job)
        return;
    const gss_trk_job_t jb = A.jobs[job];
    gss_trk_state_t t;
    if (A.first)
        gss_trk_init(&t, &jb, A.cs_nom);
    else
        t = A.state[job];
    if (t.done || t.e >= jb.n_epoch) {               /* uniform over the workgroup              */
        if (A.first && tid == 0)                     /* n_epoch 0: a later launch reads this    */
            A.state[job] = t;
        return;
    }
    load_tables(tab, A, jb.prn, NT);
    __syncthreads();
    gss_trk_rec_t *rec = A.rec + (size_t)job * A.pitch;
    const int fmt = FMT ? FMT : A.cfg.fmt;
    const int32_t e_end = jb.n_epoch - t.e > A.chunk ? t.e + A.chunk : jb.n_epoch;

    int32_t pxi[TRK_PF], pxq[TRK_PF];                /* the epoch's first samples of this lane  */
    if constexpr (!PLAIN) {
#pragma unroll
        for (int k = 0; k < TRK_PF; k++)
            sample_clamped(A, fmt, t.s + tid + k * NT, &pxi[k], &pxq[k]);
    }

    while (t.e < e_end) {
        const int32_t n = t.n_hint ? gss_trk_len_hint(t.phi, t.cs, t.n_hint)
                                   : gss_trk_len(t.phi, t.cs);
        if (t.s + n > A.N) {
            t.done = 1;
            break;
        }
        int64_t q[6] = {0, 0, 0, 0, 0, 0};
        if constexpr (PLAIN) {
            for (int32_t i = tid; i < n; i += NT) {
                int32_t xi, xq;
                gss_acq_sample(A.x, fmt, t.s + i, &xi, &xq);
                correlate(tab, xi, xq, t.phi + (int64_t)i * t.cs,
                          t.th + (uint32_t)i * (uint32_t)t.w, q);
            }
            for (int k = 0; k < 6; k++)
                slot[0][tid][k] = q[k];
            __syncthreads();
            for (int s = NT / 2; s > 0; s >>= 1) {
                if (tid < s)
                    for (int k = 0; k < 6; k++)
                        slot[0][tid][k] += slot[0][tid + s][k];
                __syncthreads();
            }
            for (int k = 0; k < 6; k++)
                q[k] = slot[0][0][k];
            __syncthreads();                         /* the slots are rewritten next epoch      */
        } else {
            int64_t c = t.phi + (int64_t)tid * t.cs;
            uint32_t th = t.th + (uint32_t)tid * (uint32_t)t.w;
            const int64_t dc = (int64_t)NT * t.cs;
            const uint32_t dth = (uint32_t)NT * (uint32_t)t.w;
            int32_t a[6] = {0, 0, 0, 0, 0, 0};
            int32_t i = tid;
#pragma unroll
            for (int k = 0; k < TRK_PF; k++) {       /* no branch: past the end counts zero     */
                correlate_any(tab, i < n ? pxi[k] : 0, i < n ? pxq[k] : 0, c, th, a);
                i += NT; c += dc; th += dth;
            }
            int held = TRK_PF;
            for (; i < n; i += TRK_U * NT) {         /* the loads of a pass first               */
                if (held + TRK_U > TRK_FLUSH) {
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        q[k] += a[k];
                        a[k] = 0;
                    }
                    held = 0;
                }
                int32_t xi[TRK_U], xq[TRK_U];
#pragma unroll
                for (int u = 0; u < TRK_U; u++)
                    sample_clamped(A, fmt, t.s + i + u * NT, &xi[u], &xq[u]);
#pragma unroll
                for (int u = 0; u < TRK_U; u++) {
                    const bool in = i + u * NT < n;
                    correlate_any(tab, in ? xi[u] : 0, in ? xq[u] : 0, c, th, a);
                    c += dc; th += dth;
                }
                held += TRK_U;
            }
            /* the next epoch's first samples, ahead of the reduction and its barrier: a sample
               of that epoch lies inside the N samples, any other is discarded */
            const int64_t s_next = t.s + n;
#pragma unroll
            for (int k = 0; k < TRK_PF; k++)
                sample_clamped(A, fmt, s_next + tid + k * NT, &pxi[k], &pxq[k]);
            const int par = t.e & 1;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const int64_t v = wave_sum(q[k] + a[k]);
                if ((tid & 63) == 0)
                    slot[par][tid >> 6][k] = v;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 6; k++) {
                int64_t v = 0;
#pragma unroll
                for (int w = 0; w < TRK_WAVES; w++)
                    v += slot[par][w][k];
                q[k] = v;
            }
        }
        gss_trk_rec_t r;
        const int32_t e = t.e;
        gss_trk_update(&t, &A.cfg, A.cs_nom, q, n, &r);
        if (tid == 0)
            rec[e] = r;
    }
    if (tid == 0) {
        A.state[job] = t;
        A.count[job] = t.e;
    }
}

}  // namespace

extern "C" int gss_track_device(gss_dev *d, const gss_trk_cfg_t *cfg, const void *d_samples,
                                int64_t N, const gss_trk_job_t *jobs, int n_job,
                                gss_trk_rec_t *d_rec, int64_t pitch, int32_t *d_count,
                                void *stream)
{
    int rc = gss_trk_check_args(cfg, N, jobs, n_job, pitch);
    if (rc)
        return rc;
    if (!d || !d_samples || !d_rec || !d_count ||
        (cfg->fmt == GSS_FMT_SC16 && ((uintptr_t)d_samples & 1)) || ((uintptr_t)d_rec & 7) ||
        ((uintptr_t)d_count & 3))
        return gss_fail(GSS_E_ARG, "invalid tracking buffers");
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");

    int chunk = TRK_CHUNK;
    const char *ce = getenv("GSS_TRK_CHUNK");                  /* tests: the state hand-over   */
    if (ce && atoi(ce) > 0 && atoi(ce) < TRK_CHUNK)
        chunk = atoi(ce);
    const char *path = getenv("GSS_TRK_PATH");                 /* read per call: tests switch it */
    const bool plain = path && strcmp(path, "plain") == 0;

    TrkArgs A;
    memset(&A, 0, sizeof A);
    A.cfg = *cfg;
    A.N = N;
    A.pitch = pitch;
    A.cs_nom = gss_trk_cs_nom(cfg->fs_hz);
    A.n_job = n_job;
    A.chunk = chunk;
    int32_t most = 0;
    for (int j = 0; j < n_job && N > 0; j++)                    /* no samples: no launch          */
        most = jobs[j].n_epoch > most ? jobs[j].n_epoch : most;

    auto &s = d->trk;                                           /* the handle's scratch          */
    hipStream_t st = (hipStream_t)stream;
    if ((rc = s.state.reserve((size_t)n_job * sizeof(gss_trk_state_t), "tracking scratch")) == 0 &&
        (rc = s.jobs.reserve((size_t)n_job * sizeof(gss_trk_job_t), "tracking scratch")) == 0) {
        /* the jobs go up synchronously: the caller's array is free on return */
        if (hipMemcpy(s.jobs.p, jobs, (size_t)n_job * sizeof *jobs, hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemsetAsync(d_count, 0, (size_t)n_job * sizeof(int32_t), st) != hipSuccess)
            rc = gss_fail(GSS_E_HIP, "tracking: %s", hipGetErrorString(hipGetLastError()));
    }
    if (rc)
        return rc;
    A.x = d_samples; A.jobs = s.jobs.p; A.state = s.state.p; A.rec = d_rec; A.count = d_count;
    A.ca = d->tab.p->ca; A.lut = d->tab.p->lut;
    for (int32_t done = 0; done < most; done += chunk) {
        A.first = done == 0;
        const dim3 grid((unsigned)n_job);
        if (plain)
            hipLaunchKernelGGL((gss_track_kernel<true, TRK_PLAIN_THREADS, 0>), grid,
                               dim3(TRK_PLAIN_THREADS), 0, st, A);
        else if (cfg->fmt == GSS_FMT_SC16)
            hipLaunchKernelGGL((gss_track_kernel<false, TRK_THREADS, GSS_FMT_SC16>), grid,
                               dim3(TRK_THREADS), 0, st, A);
        else if (cfg->fmt == GSS_FMT_SC08)
            hipLaunchKernelGGL((gss_track_kernel<false, TRK_THREADS, GSS_FMT_SC08>), grid,
                               dim3(TRK_THREADS), 0, st, A);
        else
            hipLaunchKernelGGL((gss_track_kernel<false, TRK_THREADS, GSS_FMT_SC01>), grid,
                               dim3(TRK_THREADS), 0, st, A);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "tracking kernel: %s", hipGetErrorString(e));
}

extern "C" int gss_track(gss_dev *d, const gss_trk_cfg_t *cfg, const void *samples, int64_t N,
                         const gss_trk_job_t *jobs, int n_job, gss_trk_rec_t *rec, int64_t pitch,
                         int32_t *count)
{
    int rc = gss_trk_check_args(cfg, N, jobs, n_job, pitch);
    if (rc)
        return rc;
    if (!d || !samples || !rec || !count)
        return gss_fail(GSS_E_ARG, "invalid tracking buffers");
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    const size_t nb = gss_acq_bytes(cfg->fmt, N);
    const size_t rb = (size_t)n_job * (size_t)pitch * sizeof(gss_trk_rec_t);
    const size_t cb = (size_t)n_job * sizeof(int32_t);
    void *dx = nullptr, *dr = nullptr, *dc = nullptr;
    if (hipMalloc(&dx, nb ? nb : 4) != hipSuccess || hipMalloc(&dr, rb ? rb : 8) != hipSuccess ||
        hipMalloc(&dc, cb) != hipSuccess)
        rc = gss_fail(GSS_E_NOMEM, "tracking: out of device memory");
    else if (hipMemcpy(dx, samples, nb, hipMemcpyHostToDevice) != hipSuccess)
        rc = gss_fail(GSS_E_HIP, "tracking: upload failed");
    else if ((rc = gss_track_device(d, cfg, dx, N, jobs, n_job, (gss_trk_rec_t *)dr, pitch,
                                    (int32_t *)dc, nullptr)) == 0) {
        if (hipMemcpy(count, dc, cb, hipMemcpyDeviceToHost) != hipSuccess)
            rc = gss_fail(GSS_E_HIP, "tracking: %s", hipGetErrorString(hipGetLastError()));
        for (int j = 0; j < n_job && rc == 0; j++)           /* only the records written       */
            if (count[j] > 0 &&
                hipMemcpy(rec + (size_t)j * pitch, (gss_trk_rec_t *)dr + (size_t)j * pitch,
                          (size_t)count[j] * sizeof(gss_trk_rec_t),
                          hipMemcpyDeviceToHost) != hipSuccess)
                rc = gss_fail(GSS_E_HIP, "tracking: %s", hipGetErrorString(hipGetLastError()));
    }
    (void)hipFree(dx);
    (void)hipFree(dr);
    (void)hipFree(dc);
    return rc;
}
