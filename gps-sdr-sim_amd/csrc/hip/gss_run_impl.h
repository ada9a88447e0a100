/*
 * gss_run_impl.h — what the two sides of the streaming driver share (private to csrc/hip):
 *   gss_run_plan.hip   the planner, rows and prover threads
 *   gss_run.hip        the main thread, set-up and tear-down, the entry points
 * The slots and the run's state, and the few helpers both sides use.  A slot's buffers belong to
 * exactly one side at a time (Slot::state under Run::mu).  Only the pools' interface
 * (gss_run_pool.h) and the three thread functions below have external linkage; the library's
 * export map keeps them out of its dynamic symbols.
 */
#ifndef GSS_RUN_IMPL_H
#define GSS_RUN_IMPL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <time.h>
#include <condition_variable>
#include <mutex>
#include <vector>
#include "gpssim_amd.h"
#include "gss_run_modes.h"
#include "gss_run_pool.h"
#include "gss_run_stages.h"

extern "C" void gss_pool_select(int id);             /* pool.c */
/* n bytes from src to dst by a copy kernel on st: pinned host or device memory on either side
   (gss_producers.hip; not exported) */
int run_copy_launch(void *dst, const void *src, size_t n, hipStream_t st);
int run_proof_launch(const gss_chan_blk_t *blk, const int32_t *nch, int nblk, int n_per_blk,
                     const uint32_t *ca_bits, int n_ca, const uint32_t *nav, int n_nav,
                     const gss_carr_anchor_t *anch, const gss_spec_in_t *sin,
                     const gss_spec_t *sspec, gss_lin_t *lin, int32_t *fast, int64_t first,
                     int force_exact, hipStream_t st);            /* gss_proof.hip */

#define RUN_TRY(x)                                                                           \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess)                                                                \
            return gss_fail(GSS_E_HIP, "HIP error %s at %s:%d", hipGetErrorString(e_),      \
                            __FILE__, __LINE__);                                             \
    } while (0)

/* a sequence of HIP calls up to its first failure */
#define THEN(e, x)                                                                           \
    do {                                                                                     \
        if ((e) == hipSuccess)                                                               \
            (e) = (x);                                                                       \
    } while (0)

namespace gss_run_ {

/* GSS_RUN_TRACE=1: per-slot timestamps on stderr (planner start/end, submit, drain wait/end) */
static inline double tnow()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
inline int trace_on()
{
    static int on = -1;
    if (on < 0) {
        const char *e = getenv("GSS_RUN_TRACE");
        on = e && e[0] == '1';
    }
    return on;
}

#ifndef GSS_RUN_NCOPY
#define GSS_RUN_NCOPY 1
#endif
#ifndef GSS_RUN_DEPTH
#define GSS_RUN_DEPTH 2                                /* profiles/round3/ablate_r3n.log */
#endif
constexpr int NCOPY = GSS_RUN_NCOPY;                   /* copy streams (DMA engines) */
constexpr int DEPTH = GSS_RUN_DEPTH;                   /* slots submitted, not yet drained */
#ifndef GSS_RUN_AHEAD
#define GSS_RUN_AHEAD 2
#endif
constexpr int NSLOT = DEPTH + GSS_RUN_AHEAD;           /* + slots planned / proven ahead */

enum { FREE, PROVING, PLANNED };                  /* PROVING: rows planned, proofs pending */

struct Slot {
    /* planner side (pinned host memory) */
    gss_chan_blk_t *blk = nullptr;
    int32_t *nch = nullptr;
    double *ck = nullptr;
    gss_nav_src_t *nav = nullptr;    /* sources of the nav rows new with this slot (pinned)  */
    int nav_cap = 0, n_nav = 0;      /* ... capacity, count                                   */
    int nav_first = 0;               /* global row index of the first of them                 */
    gss_lin_t *lin = nullptr;        /* certified lines [nb][GSS_MAXCH] (fast path)      */
    int32_t *fast = nullptr;         /* fast[nb], then the exact-path block list [n_fb] */
    gss_carr_anchor_t *anch = nullptr;   /* the chain's anchors [nb][GSS_MAXCH] (proofs)   */
    int has_anch = 0;                /* ... filled for this use of the slot               */
    int sb_idx = -1;                 /* records mode: the walk batch it came from (its device
                                        walks are the GPU proofs' anchors)                  */
    int n_fb = 0;
    int verdicts = 0;                /* GPU proofs: the exact-path blocks went with the render
                                        (submit_proven), no redo in drain                     */
    int nb = 0, nch_max = 1;
    int64_t first = 0;               /* run index of the slot's first block */
    const uint32_t *lin_nav = nullptr;   /* the nav table its proofs read (prover thread)  */
    int lin_n_nav = 0;
    int end = 0, err = 0;            /* last slot / planner error code      */
    int state = FREE;
    /* main side */
    uint8_t *d_in = nullptr;
    size_t d_in_cap = 0;
    uint8_t *d_out = nullptr, *h_out = nullptr;
    uint8_t *d_imp = nullptr;        /* RunStages::needs_imp_buf: the last stage's output (d_out
                                        holds the SC16 render; noise alone into SC16 is applied
                                        in place)                                            */
    int32_t *d_status = nullptr, *h_status = nullptr;
    hipEvent_t rendered = nullptr;   /* compute stream: the slot's kernels are done      */
    hipEvent_t done = nullptr;       /* copy stream: the slot's bytes are in h_out        */
    hipEvent_t tq = nullptr;         /* GSS_RUN_TRACE: the compute stream reached the slot */
    hipEvent_t tk = nullptr;         /* ... its inputs are uploaded (kernels next)        */
    hipEvent_t tc = nullptr;         /* ... the copy stream reached its download          */
    /* GPU proofs, launched by the planner (proof_ahead) */
    hipStream_t pst = nullptr;       /* the slot's proof stream                          */
    hipEvent_t navd = nullptr;       /* its nav rows are built (the planner's nav stream) */
    hipEvent_t proved = nullptr;     /* its rows are on the device and proven            */
    int gpu_proven = 0;              /* this use of the slot is proven on the GPU         */
};

struct Run {
    explicit Run(const RunModes &modes) : m(modes) {}
    const RunModes m;                /* the run's modes (gss_run_modes.h), fixed at its start */
    RunStages stages;                /* its post-render stages (gss_run_stages.h), likewise   */
    /* the run's context, set once (run_range, run_alloc) */
    gss_scn *scn;
    gss_dev *dev = nullptr;
    int ordinal = 0;                 /* the device's ordinal, for the planner thread's hipSetDevice */
    int batch, threads, n_per_blk, carrier_int;
    hipStream_t st = nullptr;        /* the compute stream                                     */
    hipStream_t cp[NCOPY] = {};      /* the copy streams                                       */
    uint32_t *d_ca = nullptr;        /* the run's device C/A table                            */
    hipStream_t nav_st = nullptr;    /* GPU proofs: the planner's stream for the slots' nav rows */
    hipEvent_t t_base = nullptr;     /* GSS_RUN_TRACE: the GPU clock's origin (compute stream) */
    hipEvent_t ca_ready = nullptr;   /* GPU proofs: the device C/A table is built (compute stream) */
    int64_t first, last;             /* [first, last) block range of the run */
    int64_t start = 0;               /* the handle's next block when the run began (an earlier
                                        run, a seek): the planner's and rows thread's cursor   */
    const gss_run_opts_t *opts;      /* carrier hand-off (gss_run_ex), or null */
    /* the front-end filter's memory: the last n_taps - 1 unfiltered SC16 samples before the next
       slot, kept on the device by the compute stream (two buffers taken in turn: a slot shorter
       than the halo keeps part of the old one) */
    struct FilterMem {
        int16_t *d_halo[2] = {nullptr, nullptr};
        int cur = -1;                /* the buffer that holds the halo; -1: none yet (zeros)    */
    } fmem;
    /* with opts->carr_in: the whole range planned up front (rows, carriers, checkpoints) */
    std::vector<gss_chan_blk_t> pre_blk;
    std::vector<int32_t> pre_nch;
    std::vector<double> pre_ck;
    int64_t pre_n = 0, pre_at = 0;
    std::mutex mu;
    std::condition_variable cv;
    int abort = 0;
    uint32_t ca[32 * GSS_CA_WORDS];  /* C/A chips (gss_ca_table) for the proofs' patch terms */
    int nav_planned = 0;             /* nav rows whose sources a slot has taken (planner)      */
    uint32_t *d_nav = nullptr;       /* the run's nav table on the device, built by the GPU   */
    size_t d_nav_cap = 0;            /* producer (gss_nav_rows_device); rows                   */
    /* the carrier chain run ahead (planner thread): two batches, so that the GPU walks of the
       next one run while this slot's proofs do */
    struct SpecBatch {
        std::vector<gss_chan_blk_t> blk;
        std::vector<int32_t> nch;
        std::vector<gss_chain_t> chain;
        gss_spec_in_t *h_in = nullptr;        /* pinned host, read and written by the lanes */
        gss_spec_t *h_spec = nullptr;
        /* records mode (r.m.rec): the walks and guesses stay on the device (d_in, d_spec) and
           only each row's record comes back (h_rec, pinned) */
        gss_spec_in_t *d_in = nullptr;
        gss_spec_t *d_spec = nullptr;
        gss_spec_rec_t *h_rec = nullptr;
        hipEvent_t consumed = nullptr;        /* a slot's GPU proof has read d_in / d_spec */
        int consumed_pending = 0;
        double carr[GSS_MAXCH];                              /* exact, at its first block */
        int nb = 0, launched = 0;
        double tg = 0.0, tk = 0.0;                           /* trace: guess start, launch end */
        hipEvent_t walked = nullptr;          /* spec stream: this batch's walks are done      */
    } sb[3];
    int sb_cur = 0;
    int sb_head = 0, n_fly = 0, fly_end = 0;   /* rows_ahead: walks in flight (FIFO from
                                                  sb_head), and whether the rows have ended */
    /* the rows produced ahead on their own thread (chain run ahead, no hand-off): during the run
       the scenario belongs to that thread; it hands over each batch's rows with the nav rows and
       sources new with it, and the planner keeps the slot carriers and host copies of the nav
       table (the proofs read it) */
    struct RowBatch {
        std::vector<gss_chan_blk_t> blk;
        std::vector<int32_t> nch;
        std::vector<gss_chain_t> chain;
        std::vector<gss_nav_src_t> nav_src;
        std::vector<uint32_t> nav_rows;
        int64_t first = 0;
        int nb = 0, end = 0, err = 0, ready = 0;
        double t0 = 0.0, t1 = 0.0;                           /* trace: production start, end */
    } rb[2];
    int rb_take = 0, rows_done = 0;
    double carr[GSS_MAXCH];          /* rows_ahead: the slot carriers at the planner's next batch */
    std::vector<gss_nav_src_t> nav_src_h;
    std::vector<uint32_t> nav_rows_h;
    hipStream_t spec_st = nullptr;   /* the walks' stream (high priority)                      */
    uint64_t *spec_warm = nullptr;   /* device scratch of the walks' first launch (one row) */
    int64_t spec_rows = 0, spec_hits = 0;
    Slot slot[NSLOT];
};

/* the threads of gss_run_plan.hip (run_range starts them): the slots' rows and proofs; with
   r->m.rows_ahead the scenario's rows a batch ahead; with r->m.prover the host proofs */
void planner(Run *r);
void rows_thread(Run *r);
void prover(Run *r);

/* a field of the run's shared state set under its mutex, and the waiters woken */
static inline void post(Run &r, int &field, int v)
{
    {
        std::lock_guard<std::mutex> lk(r.mu);
        field = v;
    }
    r.cv.notify_all();
}

/* The carrier checkpoints feed only the exact path's Stage A, i.e. the blocks the proofs do not
   certify (none of the 2,999 of the bench run).  With the fast path the chain is therefore
   walked without them (a third cheaper: no partial-cycle walks to the 8 checkpoint positions)
   and they are computed afterwards for the uncertified blocks only, from each row's carr0 by
   the same exact walk.  The integer-carrier chain records them for free and keeps doing so. */
static inline bool lazy_ck(const Run &r) { return r.m.use_lin && !r.carrier_int; }

/* Uploads of the slots' inputs (rows, lines, checkpoints, nav sources: ~10 MB per 2048-block
   slot) by a kernel reading the pinned host buffers directly, not by the copy engine
   (run_copy_launch, gss_producers.hip): an engine copy queues behind the download of the slot
   before (the same engine, FIFO), so each slot's render started only once the previous slot's
   bytes were out, and the downloads ran at 0.78 of the link (tools/d2h_overlap.py: a 10 MB
   upload issued during a 133 MB download finishes with it, 2.09 ms instead of 0.20).  The
   kernel's reads go host-to-device, the downloads device-to-host: the two directions of the
   link overlap. */
/* host buffer (pinned) to device, stream-ordered on st */
static inline int h2d(const Run &r, void *dst, const void *src, size_t n, hipStream_t st)
{
    if (n == 0 || r.m.upload_dev)
        return run_copy_launch(dst, src, n, st);
    return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st) == hipSuccess
               ? 0 : gss_fail(GSS_E_HIP, "upload of %zu B", n);
}
#define RUN_H2D(dst, src, n, st)                                                          \
    do {                                                                                  \
        int rc_ = h2d(r, (dst), (src), (n), (st));                                        \
        if (rc_) return rc_;                                                              \
    } while (0)

/* the exact-path block list fast[nb..] from the verdicts fast[0..nb): the blocks the proof
   rejected, in order; sets and returns its length (sl.n_fb) */
static inline int list_exact(Slot &sl)
{
    int nf = 0;
    for (int b = 0; b < sl.nb; b++)
        if (!sl.fast[b])
            sl.fast[sl.nb + nf++] = b;
    return sl.n_fb = nf;
}

/* the listed blocks' lazy checkpoints, from their rows' exact carriers (see lazy_ck) */
static inline void fill_lazy_ck(const Run &r, Slot &sl)
{
    if (!lazy_ck(r))
        return;
    for (int i = 0; i < sl.n_fb; i++) {
        const int b = sl.fast[sl.nb + i];
        for (int k = 0; k < sl.nch[b]; k++) {
            const size_t e = (size_t)b * GSS_MAXCH + k;
            (void)gss_carr_advance_ck(sl.blk[e].carr0, sl.blk[e].carr_step, r.n_per_blk,
                                      sl.ck + e * GSS_NCK);
        }
    }
}

/* The rows of the device nav table a slot's kernels may index: every row up to the slot's own,
   at least 1 (the table is never smaller: nav_reserve).  The count is 0 only while no block has
   had a channel, and then no kernel reads the table: the render launches ignore the count, the
   proof and echo launches check each row's index against it and have no row to check, and the
   echo launch refuses a count of 0 (gss_echo_args).  So every launch takes this count. */
static inline int slot_nav_rows(const Slot &sl)
{
    const int n = sl.nav_first + sl.n_nav;
    return n > 0 ? n : 1;
}

/* a slot's inputs on the device, one allocation (sl.d_in) */
struct SlotDev {
    gss_chan_blk_t *blk;
    int32_t *nch;
    double *ck;
    gss_nav_src_t *src;
    gss_lin_t *lin;
    int32_t *fast;                   /* fast[nb], then the exact-path block list */
    gss_carr_anchor_t *anch;         /* the chain's anchors (GPU proofs), or null */
    size_t need;
};

static inline SlotDev slot_dev(const Slot &sl)
{
    const size_t nb = (size_t)sl.nb, rows = GSS_MAXCH * nb;
    size_t off = 0;                                    /* each part 256-byte aligned */
    auto take = [&](size_t bytes) {
        uint8_t *p = sl.d_in + off;
        off += (bytes + 255) & ~(size_t)255;
        return (void *)p;
    };
    SlotDev v;
    v.blk = (gss_chan_blk_t *)take(sizeof(gss_chan_blk_t) * rows);
    v.nch = (int32_t *)take(sizeof(int32_t) * nb);
    v.ck = (double *)take(sizeof(double) * GSS_NCK * rows);
    v.src = (gss_nav_src_t *)take(sizeof(gss_nav_src_t) * (size_t)(sl.n_nav > 0 ? sl.n_nav : 1));
    v.lin = (gss_lin_t *)take(sl.lin ? sizeof(gss_lin_t) * rows : 0);
    v.fast = (int32_t *)take(sl.lin ? sizeof(int32_t) * 2 * nb : 0);
    v.anch = sl.has_anch && sl.gpu_proven
                 ? (gss_carr_anchor_t *)take(sizeof(gss_carr_anchor_t) * rows) : nullptr;
    v.need = off;
    return v;
}

/* sl.d_in holds the slot's inputs (slot_dev(sl).need), grown if it must; busy: the stream whose
   earlier work may still read the old buffer (synchronised first), or null */
static inline int slot_in_reserve(Slot &sl, hipStream_t busy)
{
    const size_t need = slot_dev(sl).need;
    if (need <= sl.d_in_cap)
        return 0;
    if (busy)
        RUN_TRY(hipStreamSynchronize(busy));
    dev_free(sl.d_in);
    sl.d_in = nullptr;
    sl.d_in_cap = 0;
    RUN_TRY(dev_alloc((void **)&sl.d_in, need));
    sl.d_in_cap = need;
    return 0;
}

}  // namespace gss_run_

#endif
