/*
 * gss_run_pool.hip — the buffer and stream pools of the streaming driver (gss_run_pool.h).  Host
 * code only: no kernel here.
 */
#include <hip/hip_runtime.h>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "gss_run_impl.h"                              /* NCOPY, NSLOT: the streams of a run */

namespace {

/* The slots' output buffers (pinned host + device, ~133 MB each at the defaults) outlive a run:
   page-locking them costs tens of ms, so a later gss_run in the same process (a service, or a
   rank's next window) takes them from this pool instead.  Bounded by POOL_MAX_BYTES (the sizes
   of the buffers themselves); a buffer is reused only for a request of at least half its size,
   and gss_dev_close frees a device's buffers (gss_run_pool_drain). */
struct PoolBuf { void *p; size_t n; int dev; bool host; };
std::mutex pool_mu;
std::vector<PoolBuf> pool;
size_t pool_bytes = 0;
constexpr size_t POOL_MAX_BYTES = (size_t)2 << 30;

/* The run's other buffers and its streams outlive it the same way (a run creates a dozen
   streams and pins ~75 MB of rows, lines and walk buffers at 2,048-block slots: most of a short
   run's start-up): pin_alloc / dev_alloc take from the buffer pool and record the
   size they got, so that pin_free / dev_free (any pointer, null included) give it back;
   stream_get / stream_put keep idle non-blocking streams per device and priority. */
std::unordered_map<void *, PoolBuf> pool_out;          /* pooled buffers in use, by pointer */
struct PoolStream { hipStream_t s; int dev; int hi; };
std::vector<PoolStream> spool;                         /* idle streams */
std::vector<PoolStream> spool_out;                     /* pooled streams in use */

/* a buffer of at least n bytes; *got = its actual size, which pool_put must be given back */
hipError_t pool_get(void **p, size_t n, bool host, int dev, size_t *got)
{
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        for (size_t i = 0; i < pool.size(); i++) {
            const PoolBuf &b = pool[i];
            if (b.host == host && b.dev == dev && b.n >= n && b.n <= 2 * n) {
                *p = b.p;
                *got = b.n;
                pool_bytes -= b.n;
                pool.erase(pool.begin() + (long)i);
                return hipSuccess;
            }
        }
    }
    *got = n;
    return host ? hipHostMalloc(p, n, hipHostMallocDefault) : hipMalloc(p, n);
}

void pool_put(void *p, size_t n, bool host, int dev)
{
    if (!p)
        return;
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        if (pool_bytes + n <= POOL_MAX_BYTES) {
            pool.push_back({p, n, dev, host});
            pool_bytes += n;
            return;
        }
    }
    (void)(host ? hipHostFree(p) : hipFree(p));
}

/* The pool's key is the calling thread's current device (hipGetDevice).  A run's threads all
   allocate on the run's device: the main thread reads it with hipGetDevice just before its
   set-up (run_range: Run::ordinal), and the planner thread sets that ordinal before its first
   allocation. */
hipError_t pooled_alloc(void **p, size_t n, bool host)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    size_t got = 0;
    *p = nullptr;
    const hipError_t e = pool_get(p, n, host, dev, &got);
    if (e == hipSuccess && *p) {
        std::lock_guard<std::mutex> lk(pool_mu);
        pool_out[*p] = {*p, got, dev, host};
    }
    return e;
}

void pooled_free(void *p)
{
    if (!p)
        return;
    PoolBuf b;
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        const auto it = pool_out.find(p);
        if (it == pool_out.end())
            return;                                    /* not a pooled buffer */
        b = it->second;
        pool_out.erase(it);
    }
    pool_put(b.p, b.n, b.host, b.dev);
}

}  // namespace

namespace gss_run_ {

hipError_t pin_alloc(void **p, size_t n) { return pooled_alloc(p, n, true); }
hipError_t dev_alloc(void **p, size_t n) { return pooled_alloc(p, n, false); }
void pin_free(void *p) { pooled_free(p); }
void dev_free(void *p) { pooled_free(p); }

hipError_t stream_get(hipStream_t *s, bool hi)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        for (size_t i = 0; i < spool.size(); i++)
            if (spool[i].dev == dev && spool[i].hi == (int)hi) {
                *s = spool[i].s;
                spool_out.push_back(spool[i]);
                spool.erase(spool.begin() + (long)i);
                return hipSuccess;
            }
    }
    hipError_t e;
    if (hi) {
        int lo_pri = 0, hi_pri = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);
        e = hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi_pri);
    } else {
        e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(pool_mu);
        spool_out.push_back({*s, dev, (int)hi});
    }
    return e;
}

void stream_put(hipStream_t s)
{
    if (!s)
        return;
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        for (size_t i = 0; i < spool_out.size(); i++)
            if (spool_out[i].s == s) {
                if (spool.size() < 64) {
                    spool.push_back(spool_out[i]);
                    spool_out.erase(spool_out.begin() + (long)i);
                    return;
                }
                spool_out.erase(spool_out.begin() + (long)i);
                break;
            }
    }
    (void)hipStreamDestroy(s);
}

}  // namespace gss_run_

/* The streams a run takes (compute, copy and nav at normal priority; the walks' and one proof
   stream per slot at the highest), made into the pool when the device opens (gss_dev_open):
   creating a high-priority stream costs ~4 ms in a fresh process, and GPU-proof runs take five
   more than host-proof runs (23 ms of a 0.7 s configs[3] run, profiles/round5/e2e/README.md) */
extern "C" void gss_run_pool_prewarm(int dev)
{
    int have[2] = {0, 0};
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        for (const PoolStream &p : spool)
            if (p.dev == dev)
                have[p.hi ? 1 : 0]++;
    }
    int lo_pri = 0, hi_pri = 0;
    if (hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri) != hipSuccess)
        return;
    const int want[2] = {2 + gss_run_::NCOPY, 1 + gss_run_::NSLOT};
    for (int hi = 0; hi < 2; hi++)
        for (; have[hi] < want[hi]; have[hi]++) {
            hipStream_t s = nullptr;
            if ((hi ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi_pri)
                    : hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess)
                return;
            std::lock_guard<std::mutex> lk(pool_mu);
            spool.push_back({s, dev, hi});
        }
}

/* free the pooled buffers and idle streams of device `dev` (gss_dev_close; -1: every device) */
extern "C" void gss_run_pool_drain(int dev)
{
    std::vector<PoolBuf> out;
    std::vector<PoolStream> sout;
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        for (size_t i = 0; i < pool.size();) {
            if (dev < 0 || pool[i].dev == dev) {
                out.push_back(pool[i]);
                pool_bytes -= pool[i].n;
                pool.erase(pool.begin() + (long)i);
            } else {
                i++;
            }
        }
        for (size_t i = 0; i < spool.size();) {
            if (dev < 0 || spool[i].dev == dev) {
                sout.push_back(spool[i]);
                spool.erase(spool.begin() + (long)i);
            } else {
                i++;
            }
        }
    }
    for (const PoolBuf &b : out)
        (void)(b.host ? hipHostFree(b.p) : hipFree(b.p));
    for (const PoolStream &q : sout)
        (void)hipStreamDestroy(q.s);
}
