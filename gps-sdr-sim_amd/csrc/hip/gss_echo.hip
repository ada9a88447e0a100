/*
 * gss_echo.hip — multipath echoes added to a render on the GPU (gss_echo_device,
 * include/gpssim_amd.h): one streaming gfx950 kernel over the SC16 samples a render wrote, in
 * place, from the channel rows that render read.  It is the stages' common shape
 * (gss_stage_dev.h: groups, edges, grid) for SC16 in place, the groups taken a tile at a time:
 *
 *   samples  a tile of 256 groups (1,024 samples) per workgroup and trip; grid-stride over the
 *            tiles
 *   rows     per tile, the live pairs (echo, channel) of the two blocks it can touch are derived
 *            once by the workgroup's first two waves (one lane per pair, compacted by a ballot)
 *            into LDS, not per thread.  A tile that touches more blocks (blocks shorter than a
 *            tile: tests) derives the rows of the others in each thread, by the same function
 *   tables   the packed cos/sin table (2 KB) and the call's C/A chips (4 KB) in LDS; the data
 *            words are read from the nav table
 *   thread   its group is taken on the buffer, so it can straddle a block boundary: the state is
 *            then seeded again from the next block's rows.  Seeding costs one 64-bit multiply
 *            per phase and the split of q by 1023 (32-bit, by constant); the next three samples
 *            are carried (gss_echo_next): no per-sample division, no scratch
 *   edges    one sample at a time through the same arithmetic, each seeded from its own index
 *   plain    GSS_ECHO_PATH=plain (read per call), and a C/A table of more than 32 rows: one sample
 *            per thread, straight from the definition and global memory (gss_echo_plain_kernel)
 * The arithmetic is csrc/common/gss_echo.h, shared with gss_echo_host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "gss_dev.h"
#include "gss_stage_dev.h"
#include "../common/gss_echo.h"

extern "C" int gss_echo_args(const gss_echo_t *echo, int n_echo, const void *blk, const void *nch,
                             int nblk, int n_per_blk, const void *ca_bits, int n_ca,
                             const void *nav, int n_nav, uint64_t sample0,
                             const void *iq);                                  /* echo.c */

namespace {

constexpr int ECHO_THREADS = STAGE_THREADS;
constexpr int ECHO_NS = StageFmt<GSS_FMT_SC16>::NS;     /* samples per thread                  */
constexpr int ECHO_TILE = ECHO_THREADS * ECHO_NS;       /* samples per workgroup and trip      */
constexpr int ECHO_BLKS = 2;                            /* blocks whose rows a tile keeps      */
constexpr int ECHO_PAIRS = GSS_MAXECHO * GSS_MAXCH;     /* one wave: a lane per pair           */
constexpr int ECHO_CA_ROWS = 32;

struct EchoArgs {
    int16_t *iq;
    const gss_chan_blk_t *blk;
    const int32_t *nch;
    const uint32_t *ca, *nav;
    const int16_t *lut;     /* cos512 then sin512 on the device (the handle's)                  */
    uint64_t sample0;       /* absolute index of block 0's first sample                         */
    uint64_t n;             /* samples: nblk * n_per_blk                                        */
    uint64_t head;          /* samples before the first whole group                             */
    uint64_t groups;        /* whole groups of 4 samples from `head` on                         */
    double rcp_n;           /* 1 / n_per_blk                                                    */
    int32_t nblk, n_per_blk, n_ca, n_nav, n_echo;
    gss_echo_t echo[GSS_MAXECHO];
};

/* (block, sample in it) of buffer index j < A.n: the quotient by the reciprocal, then made exact */
__device__ __forceinline__ void echo_locate(const EchoArgs &A, uint64_t j, int32_t *b, int32_t *s)
{
    int64_t q = (int64_t)((double)j * A.rcp_n);
    int64_t r = (int64_t)j - q * (int64_t)A.n_per_blk;
    while (r < 0) {
        r += A.n_per_blk;
        q -= 1;
    }
    while (r >= A.n_per_blk) {
        r -= A.n_per_blk;
        q += 1;
    }
    *b = (int32_t)q;
    *s = (int32_t)r;
}

__device__ __forceinline__ int32_t echo_nch(const EchoArgs &A, int32_t b)
{
    const int32_t c = A.nch[b];
    return c < 0 ? 0 : c > GSS_MAXCH ? GSS_MAXCH : c;
}

/* the row of (echo e, channel k) of block b, or 0 */
__device__ __forceinline__ int echo_pair(const EchoArgs &A, const gss_echo_t &e, int32_t b, int k,
                                         gss_echo_row_t *row)
{
    const gss_chan_blk_t r = A.blk[(size_t)b * GSS_MAXCH + k];
    return gss_echo_row(&e, &r, A.sample0 + (uint64_t)b * (uint64_t)A.n_per_blk, A.n_ca, A.n_nav,
                        row);
}

/* f(row) for every live pair of block b, derived here.  The echo's index is a constant in every
   copy of the body: a dynamic index into the kernel's arguments would put them in scratch */
template <class F> __device__ __forceinline__ void echo_pairs(const EchoArgs &A, int32_t b, F f)
{
    const int32_t nc = echo_nch(A, b);
#pragma unroll
    for (int j = 0; j < GSS_MAXECHO; j++) {
        if (j >= A.n_echo)
            break;
        for (int k = 0; k < nc; k++) {
            gss_echo_row_t row;
            if (echo_pair(A, A.echo[j], b, k, &row))
                f(row);
        }
    }
}

/* one pair over the group's samples [i0, i1), the first of them sample s of the pair's block */
__device__ __forceinline__ void echo_run(const gss_echo_row_t &row, const uint32_t *ca,
                                         const uint32_t *nav, const uint32_t *L, int32_t s, int i0,
                                         int i1, int32_t (&E)[2 * ECHO_NS])
{
    gss_echo_state_t st;
    gss_echo_seed(&row, nav, (uint32_t)s, &st);
#pragma unroll
    for (int i = 0; i < ECHO_NS; i++) {
        if (i >= i0 && i < i1) {
            gss_echo_add(&st, ca, L, &E[2 * i], &E[2 * i + 1]);
            if (i + 1 < i1)
                gss_echo_next(&row, nav, &st);
        }
    }
}

struct EchoLds {
    uint32_t L[GSS_JAM_LUT];
    uint32_t CA[ECHO_CA_ROWS * GSS_CA_WORDS];
    gss_echo_t E[GSS_MAXECHO];
    gss_echo_row_t R[ECHO_BLKS][ECHO_PAIRS];
    int32_t NP[ECHO_BLKS];
};

/* one group: 4 samples from buffer index j (16-byte aligned there); b_lo: the first block whose
   rows the tile keeps */
__device__ __forceinline__ void echo_group(const EchoArgs &A, const EchoLds &S, int32_t b_lo,
                                           uint64_t j)
{
    int4 *p = reinterpret_cast<int4 *>(A.iq + 2 * j);
    const int4 r = *p;
    const int32_t pr[4] = {r.x, r.y, r.z, r.w};
    int32_t E[2 * ECHO_NS];
#pragma unroll
    for (int i = 0; i < 2 * ECHO_NS; i++)
        E[i] = 0;
    int32_t b, s;
    echo_locate(A, j, &b, &s);
    for (int i0 = 0; i0 < ECHO_NS;) {
        const int32_t room = A.n_per_blk - s;
        const int i1 = room < ECHO_NS - i0 ? i0 + room : ECHO_NS;
        const uint32_t slot = (uint32_t)(b - b_lo);
        if (slot < (uint32_t)ECHO_BLKS) {
            const int np = S.NP[slot];
            for (int q = 0; q < np; q++) {
                const gss_echo_row_t row = S.R[slot][q];
                echo_run(row, S.CA + row.ca_tbl * GSS_CA_WORDS,
                         A.nav + (size_t)row.nav_tbl * GSS_NAV_WORDS, S.L, s, i0, i1, E);
            }
        } else {
            echo_pairs(A, b, [&](const gss_echo_row_t &row) {
                echo_run(row, S.CA + row.ca_tbl * GSS_CA_WORDS,
                         A.nav + (size_t)row.nav_tbl * GSS_NAV_WORDS, S.L, s, i0, i1, E);
            });
        }
        s = 0;
        b += 1;
        i0 = i1;
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < ECHO_NS; i++) {
        const int32_t yi = gss_echo_mix((int32_t)(int16_t)(pr[i] & 0xFFFF), E[2 * i]);
        const int32_t yq = gss_echo_mix(pr[i] >> 16, E[2 * i + 1]);
        o[i] = ((uint32_t)yi & 0xFFFFu) | ((uint32_t)yq << 16);
    }
    *p = make_int4((int)o[0], (int)o[1], (int)o[2], (int)o[3]);
}

/* one sample at buffer index j (block b, sample s), every pair seeded from s: the definition.
   ca: the C/A table ([n_ca][GSS_CA_WORDS]) wherever it lies; L: the packed table, or null for
   the handle's two tables in global memory */
__device__ __forceinline__ void echo_sample(const EchoArgs &A, const uint32_t *ca,
                                            const uint32_t *L, uint64_t j, int32_t b, int32_t s)
{
    int32_t ei = 0, eq = 0;
    echo_pairs(A, b, [&](const gss_echo_row_t &row) {
        gss_echo_state_t st;
        gss_echo_seed(&row, A.nav + (size_t)row.nav_tbl * GSS_NAV_WORDS, (uint32_t)s, &st);
        const uint32_t idx = gss_echo_cell(&st);
        const uint32_t cell = L ? L[idx] : gss_jam_cell(A.lut[idx], A.lut[GSS_JAM_LUT + idx]);
        gss_echo_add_cell(&st, ca + row.ca_tbl * GSS_CA_WORDS, cell, &ei, &eq);
    });
    A.iq[2 * j] = (int16_t)gss_echo_mix(A.iq[2 * j], ei);
    A.iq[2 * j + 1] = (int16_t)gss_echo_mix(A.iq[2 * j + 1], eq);
}

__global__ __launch_bounds__(ECHO_THREADS) void gss_echo_kernel(EchoArgs A)
{
    __shared__ EchoLds S;
    stage_fill_lut(S.L, A.lut);
    for (int i = threadIdx.x; i < A.n_ca * GSS_CA_WORDS; i += ECHO_THREADS)   /* n_ca <= 32 */
        S.CA[i] = A.ca[i];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < GSS_MAXECHO; i++)
            S.E[i] = A.echo[i];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t tiles = (A.groups + ECHO_THREADS - 1) / ECHO_THREADS;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int32_t b_lo, s_lo;
        echo_locate(A, A.head + t * ECHO_TILE, &b_lo, &s_lo);
        __syncthreads();                        /* the tables are there; the last tile is done */
        if (wave < ECHO_BLKS) {
            const int32_t b = b_lo + wave;
            gss_echo_row_t row;
            const int je = lane >> 4, k = lane & 15;
            const int live = b < A.nblk && je < A.n_echo && k < echo_nch(A, b)
                                 ? echo_pair(A, S.E[je], b, k, &row) : 0;
            const uint64_t m = __ballot(live);
            if (live)
                S.R[wave][__popcll(m & ((1ull << lane) - 1ull))] = row;
            if (lane == 0)
                S.NP[wave] = __popcll(m);
        }
        __syncthreads();
        const uint64_t g = t * ECHO_THREADS + threadIdx.x;
        if (g < A.groups)
            echo_group(A, S, b_lo, A.head + g * ECHO_NS);
    }
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * ECHO_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * ECHO_THREADS;
    for (uint64_t e = t0; e < stage_edge_items<ECHO_NS, 1>(A.n, A.groups); e += stride) {
        const uint64_t j = stage_edge_at<ECHO_NS, 1>(e, A.head, A.groups);
        int32_t b, s;
        echo_locate(A, j, &b, &s);
        echo_sample(A, S.CA, S.L, j, b, s);
    }
}

__global__ __launch_bounds__(ECHO_THREADS) void gss_echo_plain_kernel(EchoArgs A)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * ECHO_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * ECHO_THREADS;
    for (uint64_t j = t0; j < A.n; j += stride) {
        const uint64_t b = j / (uint64_t)A.n_per_blk;
        echo_sample(A, A.ca, nullptr, j, (int32_t)b, (int32_t)(j - b * (uint64_t)A.n_per_blk));
    }
}

}  // namespace

extern "C" int gss_echo_device(gss_dev *d, const gss_echo_t *echo, int n_echo,
                               const gss_chan_blk_t *blk, const int32_t *nch, int nblk,
                               int n_per_blk, const uint32_t *ca_bits, int n_ca,
                               const uint32_t *nav, int n_nav, uint64_t sample0, int16_t *iq,
                               void *stream)
{
    if (!d)
        return gss_fail(GSS_E_ARG, "invalid echo arguments");
    const int rc = gss_echo_args(echo, n_echo, blk, nch, nblk, n_per_blk, ca_bits, n_ca, nav, n_nav,
                                 sample0, iq);
    if (rc || n_echo == 0 || nblk == 0)
        return rc;
    if (hipSetDevice(d->ordinal) != hipSuccess)
        return gss_fail(GSS_E_HIP, "hipSetDevice failed");
    EchoArgs A;
    memset(&A, 0, sizeof A);
    A.iq = iq; A.blk = blk; A.nch = nch; A.ca = ca_bits; A.nav = nav; A.lut = d->tab.p->lut;
    A.sample0 = sample0;
    A.n = (uint64_t)nblk * (uint64_t)n_per_blk;
    A.rcp_n = 1.0 / (double)n_per_blk;
    A.nblk = nblk; A.n_per_blk = n_per_blk; A.n_ca = n_ca; A.n_nav = n_nav; A.n_echo = n_echo;
    for (int i = 0; i < n_echo; i++)
        A.echo[i] = echo[i];
    const char *path = getenv("GSS_ECHO_PATH");
    const bool plain = (path && strcmp(path, "plain") == 0) || n_ca > ECHO_CA_ROWS;
    if (path && *path && strcmp(path, "plain") != 0)
        return gss_fail(GSS_E_ARG, "GSS_ECHO_PATH: '%s' (plain, or unset)", path);
    hipStream_t st = (hipStream_t)stream;
    if (plain) {
        hipLaunchKernelGGL(gss_echo_plain_kernel, dim3(gss_stage_grid(A.n, 0, ECHO_THREADS)),
                           dim3(ECHO_THREADS), 0, st, A);
    } else {
        /* in place: a base that is not a multiple of 4 bytes leaves every sample to the edges */
        gss_stage_split((uintptr_t)iq, (uintptr_t)iq, A.n, GSS_FMT_SC16, &A.head, &A.groups);
        const unsigned grid = gss_stage_grid(A.groups, gss_stage_items(A.n, A.groups, GSS_FMT_SC16),
                                             ECHO_THREADS);
        hipLaunchKernelGGL(gss_echo_kernel, dim3(grid), dim3(ECHO_THREADS), 0, st, A);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : gss_fail(GSS_E_HIP, "echo kernel: %s", hipGetErrorString(e));
}
