/*
 * gss_acquire.hip — the acquisition search on the GPU (gss_acquire_device, include/gpssim_amd.h;
 * DESIGN.md §12): for every selected PRN, Doppler bin and code phase the non-coherent power of
 * the samples against the C/A replica, then the peak and the floor of each PRN.
 *
 *   gss_acq_max_kernel    max|xI|, max|xQ| for the automatic shift (the next kernel reads them
 *                         from device memory: no host sync)
 *   gss_acq_rep_kernel    the replicas as int8 +1 / -1, [32 slots][window][Lpad], zero beyond
 *                         each window's L samples and in unused slots
 *   gss_acq_wipe_kernel   unpack, carrier wipe-off and quantiser for every bin: int8 planes
 *                         [bin][I|Q][Npad], zero beyond the N samples
 *   gss_acq_corr_kernel   the hot path.  Per (bin, window) the product of the Hankel matrix
 *                         A[tau][i] = q[tau + m L + i] with the replica matrix B[i][slot]: a
 *                         workgroup owns 128 code phases of one bin, its four waves two 16-row
 *                         tiles each, and keeps the I and Q sums of both 16-slot column tiles
 *                         side by side (v_mfma_i32_16x16x64_i8; int8 x +-1 into int32 is exact).
 *                         The q segment of a chunk (128 + 1024 bytes per plane) and the replica
 *                         chunk (32 x 1024) sit in LDS; a Hankel row's 16 bytes start at any
 *                         byte, so a lane reads the five aligned dwords around them and realigns
 *                         (v_alignbyte_b32).  The VALU form (GSS_ACQ_PATH=valu) is the same
 *                         kernel with the sums as plain multiply-adds, each lane owning the
 *                         (tau, slot) pairs the matrix form leaves in its registers.
 *   gss_acq_cand_kernel   one workgroup per (bin, PRN) row of the power grid: its maximum and
 *                         lowest code phase
 *   gss_acq_peak_kernel   one workgroup per PRN: the best candidate with the tie rule, then the
 *                         floor over the peak's bin
 * The arithmetic is csrc/common/gss_acq.h, shared with the host statement gss_acquire_host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "../common/gss_acq.h"

extern "C" int gss_acq_check(const gss_acq_t *a, gss_acq_dims_t *d);        /* acquire.c */

namespace {

constexpr int ACQ_THREADS = 256;
constexpr int ACQ_NT = 2;                            /* 16-row tau tiles per wave               */
constexpr int ACQ_TB = 4 * ACQ_NT * 16;              /* code phases per workgroup (128)         */
constexpr int ACQ_LC = 1024;                         /* samples of a window per LDS chunk       */
constexpr int ACQ_SEGW = (ACQ_TB + ACQ_LC + 32) / 4 + 1;   /* dwords of q per plane in LDS      */
constexpr int ACQ_BROW = ACQ_LC + 16;                /* replica row pitch in LDS (bank spread)  */
constexpr int ACQ_SLOTS = 32;

typedef int v4i __attribute__((ext_vector_type(4)));

struct AcqArgs {
    const void *x;
    int8_t *planes;              /* [n_bin][2][Npad]                                            */
    int8_t *rep;                 /* [32][M][Lpad]                                               */
    uint64_t *rows;              /* [n_prn][n_bin][T]: the caller's grid or scratch             */
    int32_t *maxes;              /* [2]                                                         */
    uint64_t *cand_v;            /* [n_prn][n_bin]: each row's maximum ...                      */
    uint32_t *cand_t;            /* ... and its lowest code phase                               */
    int32_t *qshift_out;
    gss_acq_peak_t *peaks;
    const uint32_t *ca;          /* gss_ca_table                                                */
    const int16_t *lut;          /* cos512 then sin512                                          */
    int64_t N, Npad;
    int32_t L, Lpad, T, E, M, K, n_bin, n_prn, fs, bin_hz, fmt, qshift;
    uint8_t prn[ACQ_SLOTS];
};

__global__ __launch_bounds__(ACQ_THREADS) void gss_acq_max_kernel(AcqArgs A)
{
    __shared__ int32_t m[2];
    if (threadIdx.x < 2)
        m[threadIdx.x] = 0;
    __syncthreads();
    int32_t mi = 0, mq = 0;
    for (int64_t n = (int64_t)blockIdx.x * ACQ_THREADS + threadIdx.x; n < A.N;
         n += (int64_t)gridDim.x * ACQ_THREADS) {
        int32_t xi, xq;
        gss_acq_sample(A.x, A.fmt, n, &xi, &xq);
        xi = xi < 0 ? -xi : xi;
        xq = xq < 0 ? -xq : xq;
        mi = xi > mi ? xi : mi;
        mq = xq > mq ? xq : mq;
    }
    atomicMax(&m[0], mi);
    atomicMax(&m[1], mq);
    __syncthreads();
    if (threadIdx.x < 2)
        atomicMax(&A.maxes[threadIdx.x], m[threadIdx.x]);
}

/* one thread per (window, position in the padded window) */
__global__ __launch_bounds__(ACQ_THREADS) void gss_acq_rep_kernel(AcqArgs A)
{
    const int64_t id = (int64_t)blockIdx.x * ACQ_THREADS + threadIdx.x;
    if (id >= (int64_t)A.M * A.Lpad)
        return;
    const int32_t m = (int32_t)(id / A.Lpad), i = (int32_t)(id % A.Lpad);
    const bool live = i < A.L;
    const int32_t chip = live ? gss_acq_chip_idx((int64_t)m * A.L + i, A.fs) : 0;
    for (int s = 0; s < ACQ_SLOTS; s++) {
        int32_t v = 0;
        if (live && s < A.n_prn)
            v = gss_acq_replica(A.ca + (A.prn[s] - 1) * GSS_CA_WORDS, chip);
        A.rep[((size_t)s * A.M + m) * A.Lpad + i] = (int8_t)v;
    }
}

/* four samples of one bin per thread: a dword of each plane */
__global__ __launch_bounds__(ACQ_THREADS) void gss_acq_wipe_kernel(AcqArgs A)
{
    __shared__ int16_t lut[1024];
    for (int i = threadIdx.x; i < 1024; i += ACQ_THREADS)
        lut[i] = A.lut[i];
    __syncthreads();
    const int32_t sh = A.qshift >= 0 ? A.qshift : gss_acq_auto_shift(A.maxes[0], A.maxes[1]);
    const int bin = blockIdx.y;
    if (A.qshift_out && bin == 0 && blockIdx.x == 0 && threadIdx.x == 0)
        *A.qshift_out = sh;
    const int64_t n0 = ((int64_t)blockIdx.x * ACQ_THREADS + threadIdx.x) * 4;
    if (n0 >= A.Npad)
        return;
    const uint32_t step = gss_acq_step(bin - A.K, A.bin_hz, A.fs);
    uint32_t oi = 0, oq = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t n = n0 + j;
        int32_t qi = 0, qq = 0;
        if (n < A.N) {
            int32_t xi, xq;
            gss_acq_sample(A.x, A.fmt, n, &xi, &xq);
            const uint32_t idx = gss_acq_lut_idx(n, step);
            gss_acq_wipe(xi, xq, lut[idx], lut[512 + idx], sh, &qi, &qq);
        }
        oi |= ((uint32_t)qi & 0xFFu) << (8 * j);
        oq |= ((uint32_t)qq & 0xFFu) << (8 * j);
    }
    int8_t *pl = A.planes + (size_t)bin * 2 * A.Npad;
    *reinterpret_cast<uint32_t *>(pl + n0) = oi;
    *reinterpret_cast<uint32_t *>(pl + A.Npad + n0) = oq;
}

/* Ownership of the sums in both forms (the C/D map of the 16x16 MFMA): lane l holds, for tau
   tile t and slot tile pt, slot 16 pt + (l & 15) and code phases 16 t + 4 (l >> 4) + reg. */
template <bool MFMA>
__global__ __launch_bounds__(ACQ_THREADS) void gss_acq_corr_kernel(AcqArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t qs[2][ACQ_SEGW];
    __shared__ __attribute__((aligned(16))) uint8_t bs[ACQ_SLOTS * ACQ_BROW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int bin = blockIdx.y;
    const int tau_blk = blockIdx.x * ACQ_TB;
    const int8_t *pl = A.planes + (size_t)bin * 2 * A.Npad;
    const bool two = A.n_prn > 16;                   /* the second slot tile is in use          */
    uint64_t P[ACQ_NT][2][4];
#pragma unroll
    for (int t = 0; t < ACQ_NT; t++)
#pragma unroll
        for (int pt = 0; pt < 2; pt++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                P[t][pt][e] = 0;

    for (int m = 0; m < A.M; m++) {
        v4i S[ACQ_NT][2][2];                         /* [tau tile][slot tile][I|Q]              */
#pragma unroll
        for (int t = 0; t < ACQ_NT; t++)
#pragma unroll
            for (int pt = 0; pt < 2; pt++)
#pragma unroll
                for (int c = 0; c < 2; c++)
                    S[t][pt][c] = v4i{0, 0, 0, 0};
        for (int i0 = 0; i0 < A.L; i0 += ACQ_LC) {
            /* the q segment from the aligned dword at or below its first byte: byte j of the
               segment is LDS byte j + shb */
            const int64_t gb = tau_blk + (int64_t)m * A.L + i0;
            const int shb = (int)(gb & 3);
            const int64_t ga = gb - shb;
            __syncthreads();
            for (int j = tid; j < 2 * ACQ_SEGW; j += ACQ_THREADS) {
                const int c = j / ACQ_SEGW, jj = j % ACQ_SEGW;
                qs[c][jj] = *reinterpret_cast<const uint32_t *>(pl + (size_t)c * A.Npad + ga +
                                                                4 * jj);
            }
            for (int j = tid; j < ACQ_SLOTS * (ACQ_LC / 16); j += ACQ_THREADS) {
                const int s = j / (ACQ_LC / 16), c = j % (ACQ_LC / 16);
                *reinterpret_cast<uint4 *>(bs + s * ACQ_BROW + 16 * c) =
                    *reinterpret_cast<const uint4 *>(A.rep + ((size_t)s * A.M + m) * A.Lpad +
                                                     i0 + 16 * c);
            }
            __syncthreads();
            const int rem = A.L - i0 < ACQ_LC ? A.L - i0 : ACQ_LC;
            const int nkb = (rem + 63) / 64;         /* the replica is zero beyond the window   */
            if constexpr (MFMA) {
                for (int kb = 0; kb < nkb; kb++) {
                    const v4i b0 = *reinterpret_cast<const v4i *>(bs + r * ACQ_BROW + kb * 64 +
                                                                  16 * g);
                    const v4i b1 = *reinterpret_cast<const v4i *>(bs + (r + 16) * ACQ_BROW +
                                                                  kb * 64 + 16 * g);
#pragma unroll
                    for (int t = 0; t < ACQ_NT; t++) {
                        const int o = shb + w * (16 * ACQ_NT) + t * 16 + r + kb * 64 + 16 * g;
                        const int d0 = o >> 2;
                        const uint32_t al = (uint32_t)(o & 3);
#pragma unroll
                        for (int c = 0; c < 2; c++) {
                            uint32_t u[5];
#pragma unroll
                            for (int j = 0; j < 5; j++)
                                u[j] = qs[c][d0 + j];
                            v4i a;
                            a.x = (int)__builtin_amdgcn_alignbyte(u[1], u[0], al);
                            a.y = (int)__builtin_amdgcn_alignbyte(u[2], u[1], al);
                            a.z = (int)__builtin_amdgcn_alignbyte(u[3], u[2], al);
                            a.w = (int)__builtin_amdgcn_alignbyte(u[4], u[3], al);
                            S[t][0][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b0, S[t][0][c],
                                                                               0, 0, 0);
                            if (two)
                                S[t][1][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                                    a, b1, S[t][1][c], 0, 0, 0);
                        }
                    }
                }
            } else {
                const int8_t *qb0 = reinterpret_cast<const int8_t *>(qs[0]);
                const int8_t *qb1 = reinterpret_cast<const int8_t *>(qs[1]);
                const int8_t *bb = reinterpret_cast<const int8_t *>(bs);
                for (int i = 0; i < nkb * 64; i++) {
                    const int32_t r0 = bb[r * ACQ_BROW + i], r1 = bb[(r + 16) * ACQ_BROW + i];
#pragma unroll
                    for (int t = 0; t < ACQ_NT; t++)
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int o = shb + w * (16 * ACQ_NT) + t * 16 + 4 * g + e + i;
                            const int32_t qi = qb0[o], qq = qb1[o];
                            S[t][0][0][e] += qi * r0;
                            S[t][0][1][e] += qq * r0;
                            if (two) {
                                S[t][1][0][e] += qi * r1;
                                S[t][1][1][e] += qq * r1;
                            }
                        }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < ACQ_NT; t++)
#pragma unroll
            for (int pt = 0; pt < 2; pt++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int64_t si = S[t][pt][0][e], sq = S[t][pt][1][e];
                    P[t][pt][e] += (uint64_t)(si * si) + (uint64_t)(sq * sq);
                }
    }
#pragma unroll
    for (int t = 0; t < ACQ_NT; t++)
#pragma unroll
        for (int pt = 0; pt < 2; pt++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int slot = 16 * pt + r;
                const int tau = tau_blk + w * (16 * ACQ_NT) + t * 16 + 4 * g + e;
                if (slot < A.n_prn && tau < A.T)
                    A.rows[((size_t)slot * A.n_bin + bin) * A.T + tau] = P[t][pt][e];
            }
}

/* the workgroup's maximum of (v, c) with ties to the lowest c, left in sv[0], si[0] */
__device__ __forceinline__ void acq_block_argmax(uint64_t bv, uint32_t bi, uint64_t *sv,
                                                 uint32_t *si)
{
    const int tid = threadIdx.x;
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    for (int s = ACQ_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const uint64_t v = sv[tid + s];
            const uint32_t c = si[tid + s];
            if (v > sv[tid] || (v == sv[tid] && c < si[tid])) {
                sv[tid] = v;
                si[tid] = c;
            }
        }
        __syncthreads();
    }
}

/* one workgroup per (bin, PRN): the row's maximum and its lowest code phase */
__global__ __launch_bounds__(ACQ_THREADS) void gss_acq_cand_kernel(AcqArgs A)
{
    __shared__ uint64_t sv[ACQ_THREADS];
    __shared__ uint32_t si[ACQ_THREADS];
    const int tid = threadIdx.x;
    const size_t row = (size_t)blockIdx.y * A.n_bin + blockIdx.x;
    const uint64_t *gr = A.rows + row * A.T;
    uint64_t bv = 0;
    uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t c = tid; c < (uint32_t)A.T; c += ACQ_THREADS) {
        const uint64_t v = gr[c];
        if (v > bv || (v == bv && c < bi)) {
            bv = v;
            bi = c;
        }
    }
    acq_block_argmax(bv, bi, sv, si);
    if (tid == 0) {
        A.cand_v[row] = sv[0];
        A.cand_t[row] = si[0];
    }
}

/* one workgroup per PRN: the best candidate (ties: the lowest bin, whose candidate is already
   its lowest code phase), then the floor over that bin's row */
__global__ __launch_bounds__(ACQ_THREADS) void gss_acq_peak_kernel(AcqArgs A)
{
    __shared__ uint64_t sv[ACQ_THREADS];
    __shared__ uint32_t si[ACQ_THREADS];
    const int tid = threadIdx.x, slot = blockIdx.x;
    const uint64_t *gr = A.rows + (size_t)slot * A.n_bin * A.T;
    uint64_t bv = 0;
    uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t c = tid; c < (uint32_t)A.n_bin; c += ACQ_THREADS) {
        const uint64_t v = A.cand_v[(size_t)slot * A.n_bin + c];
        if (v > bv || (v == bv && c < bi)) {
            bv = v;
            bi = c;
        }
    }
    acq_block_argmax(bv, bi, sv, si);
    const uint64_t peak = sv[0];
    const int32_t kb = (int32_t)si[0];
    const int32_t tau = (int32_t)A.cand_t[(size_t)slot * A.n_bin + kb];
    __syncthreads();
    uint64_t fs = 0;
    uint32_t fc = 0;
    for (int32_t t = tid; t < A.T; t += ACQ_THREADS)
        if (gss_acq_floor_cell(t, tau, A.T, A.E)) {
            fs += gr[(size_t)kb * A.T + t];
            fc++;
        }
    sv[tid] = fs;
    si[tid] = fc;
    __syncthreads();
    for (int s = ACQ_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            sv[tid] += sv[tid + s];
            si[tid] += si[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        gss_acq_peak_t o;
        o.peak = peak;
        o.floor_sum = sv[0];
        o.floor_cnt = si[0];
        o.tau = tau;
        o.bin = kb - A.K;
        o.prn = A.prn[slot];
        A.peaks[slot] = o;
    }
}

}  // namespace

extern "C" int gss_acquire_device(gss_dev *d, const gss_acq_t *a, const void *d_samples,
                                  gss_acq_peak_t *d_peaks, uint64_t *d_grid, int32_t *d_qshift,
                                  void *stream)
{
    gss_acq_dims_t dm;
    int rc = gss_acq_check(a, &dm);
    if (rc)
        return rc;
    if (!d || !d_samples || !d_peaks || (a->fmt == GSS_FMT_SC16 && ((uintptr_t)d_samples & 1)) ||
        ((uintptr_t)d_peaks & 7) || ((uintptr_t)d_grid & 7) || ((uintptr_t)d_qshift & 3))
        return gss_fail(GSS_E_ARG, "invalid acquisition buffers");
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");

    AcqArgs A;
    memset(&A, 0, sizeof A);
    A.L = dm.L; A.T = dm.T; A.E = dm.E; A.M = a->n_coh; A.K = a->n_half; A.n_bin = dm.n_bin;
    A.n_prn = dm.n_prn; A.fs = a->fs_hz; A.bin_hz = a->bin_hz; A.fmt = a->fmt;
    A.qshift = a->qshift; A.N = dm.N;
    A.Lpad = (dm.L + ACQ_LC - 1) / ACQ_LC * ACQ_LC;
    /* the correlator reads ACQ_SEGW dwords (tau tile + chunk + 36 bytes) of a plane from the
       dword at or below byte tau_blk + m L + i0, which lies below M L + T */
    A.Npad = ((int64_t)A.M * dm.L + dm.T + ACQ_TB + ACQ_LC + 64 + 1023) / 1024 * 1024;
    for (int p = 0; p < dm.n_prn; p++)
        A.prn[p] = (uint8_t)dm.prn[p];

    /* the handle's scratch, grown on demand */
    auto &s = d->acq;
    const char *what = "acquisition scratch";
    if ((rc = s.maxes.reserve(2 * sizeof(int32_t), what)) != 0 ||
        (rc = s.planes.reserve((size_t)dm.n_bin * 2 * A.Npad, what)) != 0 ||
        (rc = s.rep.reserve((size_t)ACQ_SLOTS * A.M * A.Lpad, what)) != 0 ||
        (rc = s.cand.reserve((size_t)dm.n_prn * dm.n_bin * 12, what)) != 0)
        return rc;
    if (!d_grid &&
        (rc = s.rows.reserve((size_t)dm.n_prn * dm.n_bin * dm.T * sizeof(uint64_t), what)) != 0)
        return rc;
    A.x = d_samples; A.planes = s.planes.p; A.rep = s.rep.p; A.rows = d_grid ? d_grid : s.rows.p;
    A.cand_v = s.cand.p;
    A.cand_t = reinterpret_cast<uint32_t *>(s.cand.p + (size_t)dm.n_prn * dm.n_bin);
    A.maxes = s.maxes.p; A.qshift_out = d_qshift; A.peaks = d_peaks;
    A.ca = d->tab.p->ca; A.lut = d->tab.p->lut;

    const char *path = getenv("GSS_ACQ_PATH");                 /* read per call: tests switch it */
    const bool valu = path && strcmp(path, "valu") == 0;
    hipStream_t st = (hipStream_t)stream;
    if (a->qshift < 0) {
        if (hipMemsetAsync(s.maxes.p, 0, 2 * sizeof(int32_t), st) != hipSuccess)
            return gss_fail(GSS_E_HIP, "acquisition: hipMemsetAsync failed");
        int64_t gm = (dm.N + ACQ_THREADS - 1) / ACQ_THREADS;
        gm = gm > 1024 ? 1024 : gm;
        hipLaunchKernelGGL(gss_acq_max_kernel, dim3((unsigned)gm), dim3(ACQ_THREADS), 0, st, A);
    }
    hipLaunchKernelGGL(gss_acq_rep_kernel,
                       dim3((unsigned)(((int64_t)A.M * A.Lpad + ACQ_THREADS - 1) / ACQ_THREADS)),
                       dim3(ACQ_THREADS), 0, st, A);
    hipLaunchKernelGGL(gss_acq_wipe_kernel, dim3((unsigned)(A.Npad / (4 * ACQ_THREADS)), dm.n_bin),
                       dim3(ACQ_THREADS), 0, st, A);
    const dim3 cg((unsigned)((dm.T + ACQ_TB - 1) / ACQ_TB), dm.n_bin);
    if (valu)
        hipLaunchKernelGGL(gss_acq_corr_kernel<false>, cg, dim3(ACQ_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(gss_acq_corr_kernel<true>, cg, dim3(ACQ_THREADS), 0, st, A);
    hipLaunchKernelGGL(gss_acq_cand_kernel, dim3(dm.n_bin, dm.n_prn), dim3(ACQ_THREADS), 0, st, A);
    hipLaunchKernelGGL(gss_acq_peak_kernel, dim3(dm.n_prn), dim3(ACQ_THREADS), 0, st, A);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "acquisition kernels: %s", hipGetErrorString(e));
}

extern "C" int gss_acquire(gss_dev *d, const gss_acq_t *a, const void *samples,
                           gss_acq_peak_t *peaks, uint64_t *grid, int *qshift_out)
{
    gss_acq_dims_t dm;
    int rc = gss_acq_check(a, &dm);
    if (rc)
        return rc;
    if (!d || !samples || !peaks)
        return gss_fail(GSS_E_ARG, "invalid acquisition buffers");
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    const size_t nb = gss_acq_bytes(a->fmt, dm.N);
    const size_t pb = (size_t)dm.n_prn * sizeof(gss_acq_peak_t);
    const size_t gbytes = (size_t)dm.n_prn * dm.n_bin * dm.T * sizeof(uint64_t);
    void *dx = nullptr, *dp = nullptr, *dg = nullptr, *dq = nullptr;
    int32_t sh = 0;
    if (hipMalloc(&dx, nb) != hipSuccess || hipMalloc(&dp, pb) != hipSuccess ||
        hipMalloc(&dq, sizeof sh) != hipSuccess ||
        (grid && hipMalloc(&dg, gbytes) != hipSuccess))
        rc = gss_fail(GSS_E_NOMEM, "acquisition: out of device memory");
    else if (hipMemcpy(dx, samples, nb, hipMemcpyHostToDevice) != hipSuccess)
        rc = gss_fail(GSS_E_HIP, "acquisition: upload failed");
    else if ((rc = gss_acquire_device(d, a, dx, (gss_acq_peak_t *)dp, (uint64_t *)dg,
                                      (int32_t *)dq, nullptr)) == 0) {
        if (hipMemcpy(peaks, dp, pb, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(&sh, dq, sizeof sh, hipMemcpyDeviceToHost) != hipSuccess ||
            (grid && hipMemcpy(grid, dg, gbytes, hipMemcpyDeviceToHost) != hipSuccess))
            rc = gss_fail(GSS_E_HIP, "acquisition: %s", hipGetErrorString(hipGetLastError()));
        else if (qshift_out)
            *qshift_out = sh;
    }
    (void)hipFree(dx);
    (void)hipFree(dp);
    (void)hipFree(dg);
    (void)hipFree(dq);
    return rc;
}
