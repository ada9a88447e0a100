/*
 * gss_run_pool.h — the buffer and stream pools of the streaming driver (gss_run_pool.hip): what a
 * run allocates outlives it, so that the next run of the process starts without page-locking
 * memory or creating streams again.  They know nothing of a run; gss_dev_open and gss_dev_close
 * (gss_synth.hip) call gss_run_pool_prewarm and gss_run_pool_drain.
 */
#ifndef GSS_RUN_POOL_H
#define GSS_RUN_POOL_H
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gss_run_ {

/* a pinned host / device buffer of at least n bytes of the current device, from the pool where it
   holds one of n..2n bytes (first fit); the pool remembers the size it gave, so that pin_free /
   dev_free (any pointer, null included) give it back */
hipError_t pin_alloc(void **p, size_t n);
hipError_t dev_alloc(void **p, size_t n);
void pin_free(void *p);
void dev_free(void *p);

/* a non-blocking stream of the current device (hi: the highest priority) */
hipError_t stream_get(hipStream_t *s, bool hi);
/* back to the pool when it came from stream_get (the caller has synchronised it), else
   destroyed (the CU-masked streams) */
void stream_put(hipStream_t s);

}  // namespace gss_run_

/* the streams a run takes, made into the pool when the device opens (gss_dev_open) */
extern "C" void gss_run_pool_prewarm(int dev);
/* free the pooled buffers and streams of device `dev` (gss_dev_close; -1: every device) */
extern "C" void gss_run_pool_drain(int dev);

#endif
