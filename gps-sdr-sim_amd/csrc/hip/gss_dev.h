/*
 * gss_dev.h — the device handle (include/gpssim_amd.h, gss_dev) as the library's HIP sources see
 * it: the render path's buffers and event rings, the constant tables gss_dev_open uploads, and
 * the scratch of the acquisition search and of tracking.  Everything here belongs to one handle
 * and is released by gss_dev_close; a handle is not thread-safe.
 *
 * The streaming driver (gss_run.hip, gss_run_plan.hip, gss_run_pool.hip) does not include this
 * header: it is also built against the test fake's own
 * struct gss_dev and reaches the handle through gss_dev_ordinal alone.
 */
#ifndef GSS_DEV_H
#define GSS_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpssim_amd.h"
#include "../common/gss_impair.h"

extern "C" int gss_fail(int code, const char *fmt, ...);

#define HIP_TRY(x)                                                                           \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess)                                                                \
            return gss_fail(GSS_E_HIP, "HIP error %s at %s:%d", hipGetErrorString(e_),      \
                            __FILE__, __LINE__);                                             \
    } while (0)

/* A device buffer that grows on demand: a no-op when it is large enough, otherwise freed and
   allocated again (hipFree waits for the device, so work still in flight finishes first); the
   contents do not survive.  No destructor: gss_dev_close releases every buffer after
   hipSetDevice. */
template <class T> struct gss_buf {
    T *p = nullptr;
    size_t cap = 0;                      /* bytes */
    int reserve(size_t bytes, const char *what)
    {
        if (bytes <= cap)
            return 0;
        release();
        if (hipMalloc((void **)&p, bytes) != hipSuccess) {
            p = nullptr;
            return gss_fail(GSS_E_NOMEM, "%s: %zu bytes of device memory", what, bytes);
        }
        cap = bytes;
        return 0;
    }
    void release()
    {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct lut_arg { int16_t sin512[512]; int16_t cos512[512]; };

/* The constant tables as they lie in device memory.  gss_dev_open fills one on the host and
   uploads it with one copy; nothing writes it afterwards, so any thread may launch with it. */
struct gss_dev_tables {
    uint32_t lut16[1024];                /* the fast kernel's LUT: (cos, sin) f16 pairs, the
                                            second half negated; read as uint4              */
    uint32_t ca[32 * GSS_CA_WORDS];      /* gss_ca_table                                    */
    int16_t lut[1024];                   /* cos512 then sin512 (acquisition, tracking)      */
    int32_t noise[GSS_IMP_TBL];          /* gss_noise_table                                 */
};

struct gss_trk_state;                    /* csrc/common/gss_trk.h */

struct gss_dev {
    int ordinal;
    int seg_r = 1024;                    /* samples per Stage-B lane (env GSS_SEG_R)   */
    struct anchor_set {                  /* segment-start states [blocks][16][nsegp]     */
        gss_buf<double> carr, code;
        gss_buf<uint32_t> cnt;
    } set[2];                            /* two sets: Stage A of batch k+1 beside B of k  */
    static constexpr int RING = 256;
    hipEvent_t ev_a[RING][2], ev_b[RING][2];   /* start/end of each stage launch          */
    hipEvent_t ev_l[RING][2];                  /* ... and of each fast-path launch         */
    int n_a = 0, n_b = 0, n_l = 0;
    lut_arg lut;
    gss_buf<gss_dev_tables> tab;         /* on the device: only its members' addresses are
                                            taken on the host                              */
    gss_buf<uint8_t> d_in, d_out;        /* gss_synth_host's inputs and output             */
    gss_buf<double> d_cend;
    gss_buf<uint32_t> d_cbw;             /* chip-sign bit-streams (gss_cab_kernel)         */
    gss_buf<int32_t> d_status;
    /* the exact path's leftovers of a fast-path call run on their own stream beside the fast
       kernel (a few latency-bound blocks would otherwise serialise after it) */
    hipStream_t aux = nullptr;
    hipEvent_t ev_in = nullptr, ev_fb = nullptr;
    struct {                             /* gss_acquire_device                             */
        gss_buf<int8_t> planes, rep;
        gss_buf<uint64_t> rows, cand;
        gss_buf<int32_t> maxes;
    } acq;
    struct {                             /* gss_track_device                               */
        gss_buf<gss_trk_state> state;
        gss_buf<gss_trk_job_t> jobs;
    } trk;
};

#endif /* GSS_DEV_H */
