/*
 * gss_run.hip — the streaming driver: whole run (or a block range of it) from the host control
 * plane to the caller's byte sink, every stage overlapped.  Replaces the reference's block loop
 * (gpssim.c:2154-2353: refresh, sample loop, fwrite at 2276/2283/2287, 30 s updates).
 *
 *   planner thread   gss_scn_next into pinned slot buffers (+ the sources of the nav rows new
 *                    since the previous slot), then gss_linearize: the fast path's certified
 *                    lines and patches.  With the fast path (float carrier) the carrier chain
 *                    is run ahead on the GPU: the rows come without carriers
 *                    (gss_scn_next_deferred), every block's walk runs from a guess of its start
 *                    on the planner's own stream (gss_spec_device), and the serial chain on the
 *                    host takes one partial cycle per block (gss_carr_chain_spec; exact either
 *                    way, gss_phase.h); the next batch's walks run while this slot is proved.
 *                    With a carrier hand-off (gss_run_ex) the whole range's chain is run ahead
 *                    the same way, in chunks, once the carriers arrive.  GSS_RUN_SPEC=0: the
 *                    host walks every block (gss_scn_next, gss_carr_chain)
 *   main thread      per slot: async H2D; the 30 s producer builds the new nav rows of the
 *                    run's device nav table (gss_nav_rows_device; the C/A table likewise, once
 *                    per run: gss_ca_table_device); gss_synth_lin_device on the compute stream
 *                    (certified blocks on the integer fast path, the rest on Stage A + B; with
 *                    GSS_PATH=walk gss_synth_device renders every block), the post-render stages
 *                    (stages_apply), then async D2H into a pinned output buffer on the copy
 *                    stream (after an event); while the next slot renders, hands the previous
 *                    slot's bytes to the sink in run order
 *
 * Where each part lives:
 *   gss_run.hip         this file: the main thread, set-up and tear-down, the entry points
 *   gss_run_plan.hip    the planner thread, and the rows and prover threads below
 *   gss_run_impl.h      the slots and the run's state, shared by the two
 *   gss_run_modes.h     the environment switches resolved into the run's modes
 *   gss_run_stages.h    the options of the post-render stages resolved, with every refusal
 *   gss_run_pool.hip    the buffer and stream pools that outlive a run
 *
 * Slots cycle planner -> main -> sink -> planner; a slot's buffers belong to exactly one side at
 * a time (state under a mutex).  Shipped defaults (GSS_RUN_NCOPY = 1, GSS_RUN_DEPTH = 2): one
 * compute stream and one copy stream, NSLOT = DEPTH + 2 = 4 slots; DEPTH slots are submitted
 * before the oldest is handed to the sink, so the copy engine always has the next slot's D2H
 * queued behind the current one (DEPTH 1 left it idle while the next slot uploaded and
 * rendered: 12.5 vs 13.4 GS/s, profiles/round3/ablate_r3n.log).  NCOPY = 2 alternates slots over
 * two copy streams (two DMA engines on the link; measured slower, same log).  A slot's device
 * output buffer is rewritten only after its own D2H (event).
 *
 * Two more threads where the planner is the limit.  The rows thread owns the
 * scenario during the run: next_ask's batches (gss_scn_next_deferred) with the nav rows and
 * sources new with each, a batch ahead of the planner, on its own worker pool; the planner keeps
 * the slot carriers and host copies of the nav table.  The prover thread takes the slots' host
 * proofs in slot order on its own pool: planner -> PROVING -> prover -> PLANNED -> main.
 *
 * The environment switches, read once per run (gss_run_modes.h: run_env_read) and resolved in a
 * fixed order into the run's modes (run_modes_resolve, with the measurements behind the defaults).
 * T: a test switch, M: a measurement switch; the others select a supported arrangement.
 *   switch                 values (default)           selects
 *   GSS_PATH               walk (fast)                walk: every block on the exact path, no proofs
 *   GSS_RUN_SPEC           0 (1)                      0: the carrier chain walked on the host
 *   GSS_RUN_REC            0 (1)                      0: the walks, not their records, come back
 *   GSS_RUN_ANCHORS        0 (1)                   M  0: the walks that come back anchor no proofs
 *   GSS_RUN_DEV_ANCHORS    1 (0)                   M  1: GPU proofs anchored on the device walks
 *   GSS_RUN_ROWS_AHEAD     0, 1 (slots >= 1024)       the rows thread
 *   GSS_RUN_ROWS_POOL      0 (1)                   M  0: the rows thread on the planner's worker pool
 *   GSS_RUN_PROOF          host, gpu, split (auto)    where the proofs run; split: every other slot
 *   GSS_RUN_PROVER         0 (1)                   M  0: host proofs on the planner thread
 *   GSS_RUN_UPLOAD         dma (kernel)            M  dma: the slots' inputs by the copy engine
 *   GSS_RUN_SPEC_CUS       N (0)                   M  the walks' stream on N of the device's CUs
 *   GSS_RUN_RENDER_REST    set (unset)             M  with SPEC_CUS: the render stream on the others
 *   GSS_RUN_FORCE_EXACT    k (0)                   T  every k-th block of the run to the exact path
 *   GSS_RUN_LATE_VERDICTS  1 (0)                   T  the GPU proofs' rejects always redone in drain
 *                                                     (not in a filtered run: gss_run_stages.h,
 *                                                     stages_need_order)
 *   GSS_RUN_TRACE          1 (0)                   M  timestamps on stderr; cached per process
 * Compile-time: GSS_RUN_NCOPY (1), GSS_RUN_DEPTH (2), GSS_RUN_AHEAD (2).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <thread>
#include <vector>
#include "gss_run_impl.h"

/* The stages' launches (gss_impair.hip, gss_jam.hip, gss_echo.hip, gss_fir.hip) through weak
   references: a build of this file without the kernels (the CPU harness, tests/helpers) links,
   and refuses runs that ask for a stage unless it supplies a launch of its own
   (run_stages_resolve: StageLaunches). */
extern "C" __attribute__((weak)) int gss_impair_device(gss_dev *d, const gss_impair_t *p,
                                                       const int16_t *iq, uint64_t sample0,
                                                       size_t n, int fmt, void *out,
                                                       void *stream);
extern "C" __attribute__((weak)) int gss_jam_device(gss_dev *d, const gss_impair_t *p,
                                                    const gss_jam_t *jam, int n_jam,
                                                    const int16_t *iq, uint64_t sample0, size_t n,
                                                    int fmt, void *out, void *stream);
extern "C" __attribute__((weak)) int gss_echo_device(gss_dev *d, const gss_echo_t *echo, int n_echo,
                                                     const gss_chan_blk_t *blk, const int32_t *nch,
                                                     int nblk, int n_per_blk,
                                                     const uint32_t *ca_bits, int n_ca,
                                                     const uint32_t *nav, int n_nav,
                                                     uint64_t sample0, int16_t *iq, void *stream);
extern "C" __attribute__((weak)) int gss_fir_device(gss_dev *d, const gss_fir_t *fir,
                                                    const int16_t *in, const int16_t *halo,
                                                    size_t n, int fmt, void *out, void *stream);

namespace gss_run_ {
namespace {

constexpr size_t SLOT_OUT_MAX = (size_t)256 << 20;     /* pinned output bytes per slot */

/* the walks' warm-up scratch (one row): in, its device copy, the walk, the record */
constexpr size_t WARM_IN = (sizeof(gss_spec_in_t) + 255) & ~(size_t)255;
constexpr size_t WARM_SPEC = (sizeof(gss_spec_t) + 255) & ~(size_t)255;
constexpr size_t WARM_BYTES = 2 * WARM_IN + WARM_SPEC + 128;
static_assert(sizeof(gss_spec_rec_t) <= 128, "the record fits its warm-up slot");

/* Nav-table rows a run can end with: the handle's rows so far (earlier runs, seeks, the
   allocation) plus, per 30 s update the run can cross, the re-generated frame of every active
   channel and a fresh one for every channel allocation, at most 2 GSS_MAXCH (scenario.c:
   update_30s, allocate_channels) -- the reservations of the tables that must not move during
   the run (the prover's host copy, the device table with GPU proofs) */
size_t nav_rows_bound(const gss_scn *s, const gss_scn_info_t &info)
{
    const uint32_t *rows = nullptr;
    int n = 0;
    if (gss_scn_nav_table(s, &rows, &n) != 0 || n < 0)
        n = 0;
    return (size_t)n + ((size_t)info.n_blocks / 300 + 2) * 2 * GSS_MAXCH;
}

/* the device nav table holds at least `rows` rows (grown on the compute stream's order) */
int nav_reserve(Run &r, size_t rows)
{
    if (rows <= r.d_nav_cap)
        return 0;
    size_t cap = r.d_nav_cap ? 2 * r.d_nav_cap : 4096;
    while (cap < rows)
        cap *= 2;
    uint32_t *p = nullptr;
    RUN_TRY(dev_alloc((void **)&p, sizeof(uint32_t) * GSS_NAV_WORDS * cap));
    if (r.d_nav) {
        RUN_TRY(hipStreamSynchronize(r.st));           /* earlier slots' kernels read it */
        RUN_TRY(hipMemcpy(p, r.d_nav, sizeof(uint32_t) * GSS_NAV_WORDS * r.d_nav_cap,
                          hipMemcpyDeviceToDevice));
        dev_free(r.d_nav);
    }
    r.d_nav = p;
    r.d_nav_cap = cap;
    return 0;
}

/* the slot's bytes on the device, as the sink receives them */
uint8_t *slot_bytes(const Slot &sl) { return sl.d_imp ? sl.d_imp : sl.d_out; }

/* The post-render stages (r.stages: a run with an impairment) on blocks [b0, b0 + nblk) of the
   slot, rendered at SC16 into d_out, on st.  One launch per stage: the blocks' samples are
   consecutive in the run, sample0 = run block * n_per_blk. */
int stages_apply(Run &r, Slot &sl, int b0, int nblk, hipStream_t st)
{
    const RunStages &g = r.stages;
    if (stages_need_order(g) && (b0 != 0 || nblk != sl.nb))
        return gss_fail(GSS_E_STATE, "a filtered run renders whole slots only");
    const size_t ns = (size_t)r.n_per_blk * (size_t)nblk;
    int16_t *x = (int16_t *)(sl.d_out + 4 * (size_t)r.n_per_blk * (size_t)b0);
    const uint64_t s0 = (uint64_t)(sl.first + b0) * (uint64_t)r.n_per_blk;
    int rc = 0;
    /* the echoes, on the render and its rows */
    if (g.n_echo > 0) {
        const SlotDev v = slot_dev(sl);
        rc = gss_echo_device(r.dev, g.echo, g.n_echo, v.blk + (size_t)b0 * GSS_MAXCH, v.nch + b0,
                             nblk, r.n_per_blk, r.d_ca, 32, r.d_nav, slot_nav_rows(sl), s0, x, st);
        if (rc)
            return rc;
    }
    /* the jammers (which add the noise themselves) or the impairment: the last stage writes the
       run's format into the slot's bytes; before a filter, SC16 in place */
    const int fmt = g.has_fir ? GSS_FMT_SC16 : g.fmt_out;
    void *out = g.has_fir ? (void *)x : (void *)(slot_bytes(sl) + g.bb * (size_t)b0);
    rc = g.n_jam > 0 ? gss_jam_device(r.dev, g.impair, g.jam, g.n_jam, x, s0, ns, fmt, out, st)
                     : gss_impair_device(r.dev, g.impair, x, s0, ns, fmt, out, st);
    if (rc || !g.has_fir)
        return rc;
    /* the filter writes the run's format into d_imp with the samples before the slot as its
       halo, and the slot's last n_taps - 1 unfiltered samples become the next slot's halo */
    Run::FilterMem &m = r.fmem;
    const size_t keep = (size_t)(g.fir.n_taps - 1);
    const int16_t *halo = m.cur >= 0 && keep > 0 ? m.d_halo[m.cur] : nullptr;
    rc = gss_fir_device(r.dev, &g.fir, x, halo, ns, g.fmt_out, sl.d_imp, st);
    if (rc || keep == 0)
        return rc;
    const int nxt = m.cur == 0 ? 1 : 0;
    int16_t *h = m.d_halo[nxt];
    if (ns >= keep) {
        RUN_TRY(hipMemcpyAsync(h, x + 2 * (ns - keep), 4 * keep, hipMemcpyDeviceToDevice, st));
    } else {
        if (halo)
            RUN_TRY(hipMemcpyAsync(h, halo + 2 * ns, 4 * (keep - ns), hipMemcpyDeviceToDevice, st));
        else
            RUN_TRY(hipMemsetAsync(h, 0, 4 * (keep - ns), st));
        RUN_TRY(hipMemcpyAsync(h + 2 * (keep - ns), x, 4 * ns, hipMemcpyDeviceToDevice, st));
    }
    m.cur = nxt;
    return 0;
}

/* The exact-path list of a slot proven on the GPU, to the device on st: the nf listed blocks'
   lazy checkpoints (the host proofs fill theirs, prove_host), the checkpoints, the list */
int upload_exact(const Run &r, Slot &sl, const SlotDev &v, int nf, hipStream_t st)
{
    fill_lazy_ck(r, sl);
    RUN_H2D(v.ck, sl.ck, sizeof(double) * GSS_MAXCH * GSS_NCK * (size_t)sl.nb, st);
    RUN_H2D(v.fast + sl.nb, sl.fast + sl.nb, sizeof(int32_t) * (size_t)nf, st);
    return 0;
}

/* The slot's render on st, its status cleared first: the fast path with the nf listed blocks on
   the exact path, or without lines (GSS_PATH=walk) every block on the exact path */
int slot_render(Run &r, Slot &sl, const SlotDev &v, int nf, hipStream_t st)
{
    const int fmt = r.stages.fmt;
    RUN_TRY(hipMemsetAsync(sl.d_status, 0, sizeof(int32_t), st));
    if (!sl.lin)
        return gss_synth_device(r.dev, v.blk, v.nch, sl.nch_max, v.ck, r.d_ca, 32, r.d_nav,
                                slot_nav_rows(sl), sl.nb, r.n_per_blk, fmt, sl.d_out, nullptr,
                                sl.d_status, st);
    return gss_synth_lin_device(r.dev, v.blk, v.nch, sl.nch_max, v.lin, v.fast, v.fast + sl.nb, nf,
                                v.ck, r.d_ca, 32, r.d_nav, slot_nav_rows(sl), sl.nb, r.n_per_blk,
                                fmt, sl.d_out, sl.d_status, st);
}

/* The rendered slot to the host: once the compute stream's work so far is done (rendered), the
   copy stream cp takes its bytes, its status and, with GPU proofs, the verdicts (d_verdicts, or
   null) into the pinned buffers, then records done */
int slot_download(Run &r, Slot &sl, hipStream_t cp, const int32_t *d_verdicts)
{
    RUN_TRY(hipEventRecord(sl.rendered, r.st));
    RUN_TRY(hipStreamWaitEvent(cp, sl.rendered, 0));
    if (sl.tc)
        RUN_TRY(hipEventRecord(sl.tc, cp));
    RUN_TRY(hipMemcpyAsync(sl.h_out, slot_bytes(sl), r.stages.bb * (size_t)sl.nb,
                           hipMemcpyDeviceToHost, cp));
    RUN_TRY(hipMemcpyAsync(sl.h_status, sl.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, cp));
    if (d_verdicts)
        RUN_TRY(hipMemcpyAsync(sl.fast, d_verdicts, sizeof(int32_t) * (size_t)sl.nb,
                               hipMemcpyDeviceToHost, cp));
    RUN_TRY(hipEventRecord(sl.done, cp));
    return 0;
}

/* submit for a slot proven by proof_ahead: render (every block as certified; the rejected ones
   are redone in drain), then the bytes, the status and the proofs' verdicts to the host */
int submit_proven(Run &r, Slot &sl, hipStream_t cp)
{
    const hipStream_t st = r.st;
    const SlotDev v = slot_dev(sl);
    const bool ordered = stages_need_order(r.stages);   /* never defers the verdicts: no redo */
    if (ordered)
        RUN_TRY(hipEventSynchronize(sl.proved));
    RUN_TRY(hipStreamWaitEvent(st, sl.proved, 0));
    /* the proof done (it ran ahead): its verdicts are on the host, and the blocks it rejected
       (rare) render on the exact path beside the certified ones, as with host proofs; else the
       verdicts come back with the bytes and drain redoes the rejected blocks */
    int nf = 0;
    sl.verdicts = 0;
    const hipError_t q = ordered ? hipSuccess
                         : r.m.late_verdicts ? hipErrorNotReady : hipEventQuery(sl.proved);
    if (q == hipSuccess) {
        nf = list_exact(sl);
        int rc = nf > 0 ? upload_exact(r, sl, v, nf, st) : 0;
        if (rc)
            return rc;
        sl.verdicts = 1;
    } else if (q != hipErrorNotReady) {
        return gss_fail(GSS_E_HIP, "proof event query: %s", hipGetErrorString(q));
    }
    int rc = slot_render(r, sl, v, nf, st);
    if (!rc && r.stages.impair)
        rc = stages_apply(r, sl, 0, sl.nb, st);
    if (rc)
        return rc;
    return slot_download(r, sl, cp, v.fast);
}

int submit(Run &r, Slot &sl, hipStream_t cp)
{
    const hipStream_t st = r.st;
    /* the slot's previous D2H must have read d_out before the kernels rewrite it */
    RUN_TRY(hipStreamWaitEvent(st, sl.done, 0));
    if (sl.tq)
        RUN_TRY(hipEventRecord(sl.tq, st));
    if (sl.lin && sl.gpu_proven)
        return submit_proven(r, sl, cp);
    int rc = slot_in_reserve(sl, st);
    if (rc)
        return rc;
    const double tq0 = trace_on() ? tnow() : 0.0;
    const SlotDev v = slot_dev(sl);
    RUN_H2D(v.blk, sl.blk, sizeof(gss_chan_blk_t) * GSS_MAXCH * (size_t)sl.nb, st);
    RUN_H2D(v.nch, sl.nch, sizeof(int32_t) * (size_t)sl.nb, st);
    RUN_H2D(v.ck, sl.ck, sizeof(double) * GSS_MAXCH * GSS_NCK * (size_t)sl.nb, st);
    /* the 30 s producer: this slot's new nav rows built on the device (gss_producers.hip); with
       GPU proofs in the run the planner has built them already (proof_ahead) */
    rc = r.m.gpu_proof ? 0 : nav_reserve(r, (size_t)slot_nav_rows(sl));
    if (rc)
        return rc;
    if (r.m.gpu_proof) {
        RUN_TRY(hipStreamWaitEvent(st, sl.navd, 0));
    } else if (sl.n_nav > 0) {
        RUN_H2D(v.src, sl.nav, sizeof(gss_nav_src_t) * (size_t)sl.n_nav, st);
        rc = gss_nav_rows_device(r.dev, v.src, sl.nav_first, sl.n_nav, r.d_nav, st);
        if (rc)
            return rc;
    }
    const double tq1 = trace_on() ? tnow() : 0.0;
    if (sl.lin) {                        /* the host proof's lines, verdicts and exact-path list */
        RUN_H2D(v.lin, sl.lin, sizeof(gss_lin_t) * GSS_MAXCH * (size_t)sl.nb, st);
        RUN_H2D(v.fast, sl.fast, sizeof(int32_t) * (size_t)(sl.nb + sl.n_fb), st);
        if (sl.tk)
            RUN_TRY(hipEventRecord(sl.tk, st));
    }
    rc = slot_render(r, sl, v, sl.n_fb, st);
    if (!rc && r.stages.impair)
        rc = stages_apply(r, sl, 0, sl.nb, st);
    if (rc)
        return rc;
    const double tq2 = trace_on() ? tnow() : 0.0;
    rc = slot_download(r, sl, cp, nullptr);
    if (rc)
        return rc;
    if (trace_on())
        fprintf(stderr, "trace submit_parts start %.6f h2d %.6f render %.6f out %.6f\n", tq0, tq1, tq2,
                tnow());
    return 0;
}

/* GPU proofs: the blocks they rejected (fast[b] == 0, rare: none in the bench runs) rendered
   again on the exact path alone (their checkpoints from the rows' exact carriers; the fast
   flags zeroed on the device, so that the fast kernel renders nothing), and only their bytes
   copied to the host again; synchronous */
int redo_rejected(Run &r, Slot &sl)
{
    const hipStream_t st = r.st;
    const size_t bb = r.stages.bb;
    const int nf = list_exact(sl);
    if (nf == 0)
        return 0;
    if (stages_need_order(r.stages))
        return gss_fail(GSS_E_STATE, "a filtered run cannot render blocks again");
    const SlotDev v = slot_dev(sl);
    int rc = upload_exact(r, sl, v, nf, st);
    if (rc)
        return rc;
    RUN_TRY(hipMemsetAsync(v.fast, 0, sizeof(int32_t) * (size_t)sl.nb, st));
    rc = slot_render(r, sl, v, nf, st);
    if (rc)
        return rc;
    for (int i = 0; i < nf;) {                       /* runs of consecutive rejected blocks */
        const int b0 = sl.fast[sl.nb + i];
        int j = i + 1;
        while (j < nf && sl.fast[sl.nb + j] == b0 + (j - i))
            j++;
        if (r.stages.impair && (rc = stages_apply(r, sl, b0, j - i, st)) != 0)
            return rc;
        RUN_TRY(hipMemcpyAsync(sl.h_out + bb * (size_t)b0, slot_bytes(sl) + bb * (size_t)b0,
                               bb * (size_t)(j - i), hipMemcpyDeviceToHost, st));
        i = j;
    }
    RUN_TRY(hipMemcpyAsync(sl.h_status, sl.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RUN_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < nf; i++)                      /* (the verdicts stay on the host copy) */
        sl.fast[sl.fast[sl.nb + i]] = 0;
    if (trace_on())
        fprintf(stderr, "trace redo first %lld blocks %d\n", (long long)sl.first, nf);
    return 0;
}

int drain(Run &r, Slot &sl, gss_sink_fn sink, void *user)
{
    const double t0 = trace_on() ? tnow() : 0.0;
    RUN_TRY(hipEventSynchronize(sl.done));
    const double t1 = trace_on() ? tnow() : 0.0;
    if (sl.lin && sl.gpu_proven && !sl.verdicts && !*sl.h_status) {
        int rc = redo_rejected(r, sl);
        if (rc)
            return rc;
    }
    if (*sl.h_status)
        return gss_fail(GSS_E_RANGE, "nav word index ran past dwrd[59]");
    if (sink(user, sl.h_out, r.stages.bb * (size_t)sl.nb, sl.first, sl.nb))
        return gss_fail(GSS_E_IO, "sink failed at block %lld", (long long)sl.first);
    if (trace_on()) {
        fprintf(stderr, "trace drain first %lld wait %.6f %.6f sink_end %.6f\n",
                (long long)sl.first, t0, t1, tnow());
        float a = 0, k = 0, b = 0, c = 0, q = 0;       /* GPU clock: ms since the run's base */
        if (sl.tq && r.t_base && hipEventElapsedTime(&a, r.t_base, sl.tq) == hipSuccess &&
            hipEventElapsedTime(&b, r.t_base, sl.rendered) == hipSuccess &&
            hipEventElapsedTime(&c, r.t_base, sl.done) == hipSuccess) {
            if (!sl.lin || sl.gpu_proven || hipEventElapsedTime(&k, r.t_base, sl.tk) != hipSuccess)
                k = a;
            if (hipEventElapsedTime(&q, r.t_base, sl.tc) != hipSuccess)
                q = b;
            fprintf(stderr, "trace gpu first %lld start %.3f kernels %.3f rendered %.3f done %.3f "
                    "copy %.3f\n", (long long)sl.first, a, k, b, c, q);
        }
    }
    post(r, sl.state, FREE);
    return 0;
}

/* GSS_RUN_SPEC_CUS=N (measurement): the walks' stream on N of the device's CUs, spread over
   them (every (ncu / N)-th), and with GSS_RUN_RENDER_REST=1 the render stream on the others */
hipError_t cu_mask_stream(hipStream_t *st, int n_sel, bool rest)
{
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        ncu <= 0 || n_sel <= 0 || n_sel >= ncu)
        return hipErrorInvalidValue;
    const int every = ncu / n_sel;
    std::vector<uint32_t> m((size_t)(ncu + 31) / 32, 0u);
    for (int i = 0; i < ncu; i++)
        if ((i % every == 0) != rest)
            m[(size_t)i / 32] |= 1u << (i % 32);
    return hipExtStreamCreateWithCUMask(st, (uint32_t)m.size(), m.data());
}

int run_main(Run &r, gss_sink_fn sink, void *user)
{
    int pending[DEPTH], np = 0, head = 0;              /* submitted, not yet drained (FIFO) */
    for (int i = 0;; i++) {
        Slot &sl = r.slot[i % NSLOT];
        {
            std::unique_lock<std::mutex> lk(r.mu);
            r.cv.wait(lk, [&] { return sl.state == PLANNED; });
        }
        if (sl.end) {
            int rc = 0;
            for (; np > 0 && rc == 0; np--, head = (head + 1) % DEPTH)
                rc = drain(r, r.slot[pending[head]], sink, user);
            return sl.err ? sl.err : rc;
        }
        if (np == DEPTH) {                             /* oldest slot out to the sink */
            int rc = drain(r, r.slot[pending[head]], sink, user);
            if (rc)
                return rc;
            head = (head + 1) % DEPTH;
            np--;
        }
        const double ts0 = trace_on() ? tnow() : 0.0;
        int rc = submit(r, sl, r.cp[i % NCOPY]);
        if (trace_on())
            fprintf(stderr, "trace submit slot %d %.6f %.6f\n", i % NSLOT, ts0, tnow());
        if (rc)
            return rc;
        pending[(head + np) % DEPTH] = i % NSLOT;
        np++;
    }
}

/* Set-up and teardown: each owner's allocation beside its release.  An alloc returns at its
   first failure; tear_down then releases whatever was made (every release takes nulls).  The
   order of the allocations and of the releases is the buffer and stream pools' order
   (gss_run_pool.hip: first fit): the next run of the process finds them as this one left them. */

/* The run's streams and its device C/A table, built on the compute stream by the 30 s producer
   (gss_producers.hip; r.ca is the proofs' copy on the host).  The device nav table (nav_reserve)
   goes with the C/A table. */
int run_alloc(Run &r)
{
    gss_ca_table(r.ca);
    hipError_t e = dev_alloc((void **)&r.d_ca, sizeof r.ca);
    for (int i = 0; i < 2 && r.stages.has_fir; i++)
        THEN(e, dev_alloc((void **)&r.fmem.d_halo[i], 4 * (size_t)GSS_MAXTAP));
    THEN(e, r.m.render_rest ? cu_mask_stream(&r.st, r.m.spec_cus, true) : stream_get(&r.st, false));
    for (hipStream_t &c : r.cp)
        THEN(e, stream_get(&c, false));
    if (trace_on()) {
        THEN(e, hipEventCreate(&r.t_base));
        THEN(e, hipEventRecord(r.t_base, r.st));
    }
    if (e != hipSuccess)
        return gss_fail(GSS_E_HIP, "run setup failed");
    return gss_ca_table_device(r.dev, r.d_ca, r.st);
}

void run_release_tables(Run &r)
{
    dev_free(r.d_ca);
    dev_free(r.d_nav);
    dev_free(r.fmem.d_halo[0]);
    dev_free(r.fmem.d_halo[1]);
}

void run_release_streams(Run &r)
{
    stream_put(r.st);
    for (hipStream_t c : r.cp)
        stream_put(c);
    if (r.t_base) (void)hipEventDestroy(r.t_base);
}

/* A slot's buffers and events.  Three more come later and leave with the rest: nav
   (take_nav_sources), d_in (slot_in_reserve) and anch (spec_alloc). */
int slot_alloc(const Run &r, Slot &sl)
{
    const size_t nb = (size_t)r.batch;
    const RunStages &g = r.stages;
    const unsigned ev = trace_on() ? hipEventDefault : hipEventDisableTiming;
    hipError_t e = pin_alloc((void **)&sl.blk, sizeof(gss_chan_blk_t) * GSS_MAXCH * nb);
    THEN(e, pin_alloc((void **)&sl.nch, sizeof(int32_t) * nb));
    THEN(e, pin_alloc((void **)&sl.ck, sizeof(double) * GSS_MAXCH * GSS_NCK * nb));
    THEN(e, pin_alloc((void **)&sl.h_out, g.bb * nb));
    THEN(e, pin_alloc((void **)&sl.h_status, sizeof(int32_t)));
    THEN(e, dev_alloc((void **)&sl.d_out, g.bb_r * nb));
    if (g.needs_imp_buf)
        THEN(e, dev_alloc((void **)&sl.d_imp, g.bb * nb));
    THEN(e, dev_alloc((void **)&sl.d_status, sizeof(int32_t)));
    THEN(e, hipEventCreateWithFlags(&sl.done, ev));
    THEN(e, hipEventCreateWithFlags(&sl.rendered, ev));
    if (trace_on()) {
        THEN(e, hipEventCreate(&sl.tq));
        THEN(e, hipEventCreate(&sl.tk));
        THEN(e, hipEventCreate(&sl.tc));
    }
    if (e != hipSuccess)
        return gss_fail(GSS_E_NOMEM, "run buffers (%zu B per slot)", g.bb * nb);
    if (r.m.use_lin) {
        THEN(e, pin_alloc((void **)&sl.lin, sizeof(gss_lin_t) * GSS_MAXCH * nb));
        THEN(e, pin_alloc((void **)&sl.fast, sizeof(int32_t) * 2 * nb));
        if (e != hipSuccess)
            return gss_fail(GSS_E_NOMEM, "run lines (%zu B per slot)",
                            sizeof(gss_lin_t) * GSS_MAXCH * nb);
    }
    return 0;
}

void slot_release(Slot &sl)
{
    pin_free(sl.blk); pin_free(sl.nch); pin_free(sl.ck);
    pin_free(sl.nav); pin_free(sl.h_status);
    pin_free(sl.h_out); dev_free(sl.d_out); dev_free(sl.d_imp);
    pin_free(sl.lin); pin_free(sl.fast); pin_free(sl.anch);
    dev_free(sl.d_in); dev_free(sl.d_status);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.rendered) (void)hipEventDestroy(sl.rendered);
    if (sl.tq) (void)hipEventDestroy(sl.tq);
    if (sl.tk) (void)hipEventDestroy(sl.tk);
    if (sl.tc) (void)hipEventDestroy(sl.tc);
}

/* a batch of the chain run ahead: its rows, and the walkers' buffers (records mode: the walks
   stay on the device and the records come back; else the walks come back) */
int spec_batch_alloc(const Run &r, Run::SpecBatch &b)
{
    const size_t nb = (size_t)r.batch, rows = nb * GSS_MAXCH;
    b.blk.resize(rows);
    b.nch.resize(nb);
    b.chain.resize(rows);
    hipError_t e = hipEventCreateWithFlags(&b.walked, hipEventDisableTiming);
    THEN(e, hipEventCreateWithFlags(&b.consumed, hipEventDisableTiming));
    THEN(e, pin_alloc((void **)&b.h_in, sizeof(gss_spec_in_t) * rows));
    if (r.m.rec) {
        THEN(e, dev_alloc((void **)&b.d_in, sizeof(gss_spec_in_t) * rows));
        THEN(e, dev_alloc((void **)&b.d_spec, sizeof(gss_spec_t) * rows));
        THEN(e, pin_alloc((void **)&b.h_rec, sizeof(gss_spec_rec_t) * rows));
    } else {
        THEN(e, pin_alloc((void **)&b.h_spec, sizeof(gss_spec_t) * rows));
    }
    return e == hipSuccess ? 0
                           : gss_fail(GSS_E_NOMEM, "run carrier-chain buffers (%zu rows)", rows);
}

void spec_batch_release(Run::SpecBatch &b)
{
    pin_free(b.h_in); pin_free(b.h_spec); pin_free(b.h_rec);
    dev_free(b.d_in); dev_free(b.d_spec);
    if (b.walked) (void)hipEventDestroy(b.walked);
    if (b.consumed) (void)hipEventDestroy(b.consumed);
}

/* the chain run ahead (r.m.spec): the walks' stream, their warm-up scratch, the batches, and the
   slots' anchors for the proofs' carrier walks */
int spec_alloc(Run &r)
{
    /* high priority: the walks wait for free CUs behind the render kernels otherwise */
    hipError_t e = r.m.spec_cus > 0 ? cu_mask_stream(&r.spec_st, r.m.spec_cus, false)
                                    : stream_get(&r.spec_st, true);
    THEN(e, dev_alloc((void **)&r.spec_warm, WARM_BYTES));
    if (e != hipSuccess)
        return gss_fail(GSS_E_HIP, "run carrier-chain stream");
    for (Run::SpecBatch &b : r.sb) {
        const int rc = spec_batch_alloc(r, b);
        if (rc)
            return rc;
    }
    const size_t rows = (size_t)r.batch * GSS_MAXCH;
    if (r.m.anchors)
        for (Slot &sl : r.slot)
            if (pin_alloc((void **)&sl.anch, sizeof(gss_carr_anchor_t) * rows) != hipSuccess)
                return gss_fail(GSS_E_NOMEM, "run anchors (%zu rows)", rows);
    return 0;
}

void spec_release(Run &r)
{
    if (r.spec_st) (void)hipStreamSynchronize(r.spec_st);   /* before its batches go */
    for (Run::SpecBatch &b : r.sb)
        spec_batch_release(b);
    dev_free(r.spec_warm);
    stream_put(r.spec_st);
}

/* rows ahead (r.m.rows_ahead): the rows thread's batches and the planner's slot carriers; host
   memory only, released with the Run */
int rows_alloc(Run &r, const gss_scn_info_t &info)
{
    const size_t nb = (size_t)r.batch;
    /* the nav table's host copy never moves while the prover reads it (take_rows still grows it
       safely if the bound were passed) */
    r.nav_rows_h.reserve(nav_rows_bound(r.scn, info) * GSS_NAV_WORDS);
    for (Run::RowBatch &q : r.rb) {
        q.blk.resize(nb * GSS_MAXCH);
        q.nch.resize(nb);
        q.chain.resize(nb * GSS_MAXCH);
    }
    return gss_scn_carrier(r.scn, r.carr);
}

/* GPU proofs (r.m.gpu_proof), run ahead on the slots' own streams (proof_ahead): those streams
   and their events, the planner's nav stream, and the device nav table reserved for the whole run
   (nav_rows_bound; released with the run's tables) */
int proof_alloc(Run &r, const gss_scn_info_t &info, double t_reserve)
{
    if (stream_get(&r.nav_st, false) != hipSuccess)
        return gss_fail(GSS_E_HIP, "run nav stream");
    for (Slot &sl : r.slot) {
        hipError_t e = stream_get(&sl.pst, true);
        THEN(e, hipEventCreateWithFlags(&sl.navd, hipEventDisableTiming));
        THEN(e, hipEventCreateWithFlags(&sl.proved, hipEventDisableTiming));
        if (e != hipSuccess)
            return gss_fail(GSS_E_HIP, "run proof streams");
    }
    const double t_pst = trace_on() ? tnow() : 0.0;
    const int rc = nav_reserve(r, nav_rows_bound(r.scn, info));
    if (rc)
        return rc;
    /* the C/A table (built on the compute stream, run_alloc) before any proof stream reads it:
       an event the proof streams wait for (a host wait here held the start-up for the table's
       first kernel, ~20 ms in a fresh process) */
    hipError_t e = hipEventCreateWithFlags(&r.ca_ready, hipEventDisableTiming);
    THEN(e, hipEventRecord(r.ca_ready, r.st));
    for (Slot &sl : r.slot)
        THEN(e, hipStreamWaitEvent(sl.pst, r.ca_ready, 0));
    if (e != hipSuccess)
        return gss_fail(GSS_E_HIP, "run set-up");
    if (trace_on())
        fprintf(stderr, "trace setup_proofs streams %.6f nav_ca %.6f\n", t_pst - t_reserve,
                tnow() - t_pst);
    return 0;
}

void proof_release(Run &r)
{
    for (Slot &sl : r.slot) {
        stream_put(sl.pst);
        if (sl.navd) (void)hipEventDestroy(sl.navd);
        if (sl.proved) (void)hipEventDestroy(sl.proved);
    }
    stream_put(r.nav_st);
    if (r.ca_ready) (void)hipEventDestroy(r.ca_ready);
}

int set_up(Run &r, const gss_scn_info_t &info, double t_enter)
{
    int rc = run_alloc(r);
    for (Slot &sl : r.slot)
        if (!rc)
            rc = slot_alloc(r, sl);
    const double t_slots = trace_on() ? tnow() : 0.0;
    if (!rc && r.m.spec)
        rc = spec_alloc(r);
    if (!rc && r.m.rows_ahead)
        rc = rows_alloc(r, info);
    const double t_rows = trace_on() ? tnow() : 0.0;
    if (!rc)
        rc = gss_dev_reserve(r.dev, r.batch, r.n_per_blk);
    const double t_reserve = trace_on() ? tnow() : 0.0;
    if (trace_on())
        fprintf(stderr, "trace setup_parts slots %.6f spec_rows %.6f reserve %.6f\n",
                t_slots - t_enter, t_rows - t_slots, t_reserve - t_rows);
    if (!rc && r.m.gpu_proof)
        rc = proof_alloc(r, info, t_reserve);
    return rc;
}

/* Every stream that may still touch a slot's memory is synchronised before the slots go, the
   walks' stream before its batches (spec_release); the run's own streams go back last. */
void tear_down(Run &r)
{
    if (r.st) (void)hipStreamSynchronize(r.st);
    for (hipStream_t c : r.cp)
        if (c) (void)hipStreamSynchronize(c);
    if (r.nav_st) (void)hipStreamSynchronize(r.nav_st);
    for (Slot &sl : r.slot)                            /* proofs run ahead, not yet rendered */
        if (sl.pst) (void)hipStreamSynchronize(sl.pst);
    for (Slot &sl : r.slot)
        slot_release(sl);
    proof_release(r);
    run_release_tables(r);
    spec_release(r);
    if (trace_on() && r.spec_rows)
        fprintf(stderr, "trace spec total rows %lld hits %lld\n", (long long)r.spec_rows,
                (long long)r.spec_hits);
    run_release_streams(r);
}

/* the walks' first launch costs ~1 ms (the kernel's first use): here, on one zero row, while
   the planner produces its first rows, instead of inside its first batch */
void warm_walks(Run &r)
{
    uint8_t *w = (uint8_t *)r.spec_warm;
    (void)hipMemsetAsync(r.spec_warm, 0, WARM_BYTES, r.spec_st);
    (void)gss_spec_device(r.dev, (gss_spec_in_t *)w, 1, r.n_per_blk,
                          (gss_spec_t *)(w + 2 * WARM_IN), r.spec_st);
    if (!r.m.rec)
        return;
    (void)hipMemsetAsync(r.spec_warm, 0, WARM_BYTES, r.spec_st);
    (void)gss_spec_records_device(r.dev, (gss_spec_in_t *)w, 1, r.n_per_blk,
                                  (gss_spec_in_t *)(w + WARM_IN), (gss_spec_t *)(w + 2 * WARM_IN),
                                  (gss_spec_rec_t *)(w + 2 * WARM_IN + WARM_SPEC), r.spec_st);
}

/* the sink of a filtered range: the blocks before `first`, rendered for the filter's memory
   alone (RunStages::lead_blocks), are kept from the caller's sink */
struct TrimSink {
    gss_sink_fn sink;
    void *user;
    int64_t first;
    size_t bb;
};

int trim_sink(void *user, const void *bytes, size_t n, int64_t first_block, int nblocks)
{
    const TrimSink *t = (const TrimSink *)user;
    int64_t skip = t->first - first_block;
    skip = skip < 0 ? 0 : skip > nblocks ? nblocks : skip;
    if (skip == nblocks)
        return 0;
    return t->sink(t->user, (const uint8_t *)bytes + t->bb * (size_t)skip, n - t->bb * (size_t)skip,
                   first_block + skip, nblocks - (int)skip);
}

/* blocks [first_block, first_block + n_blocks) through the stages `stages` to the sink; opts:
   the carrier hand-off alone (the stage options are resolved) */
int run_range(gss_dev *d, gss_scn *s, int64_t first_block, int64_t n_blocks, int batch, int threads,
              gss_sink_fn sink, void *user, const gss_run_opts_t *opts, const gss_scn_info_t &info,
              const RunStages &stages, double t_enter)
{
    if (batch <= 0)
        batch = 100;
    if ((size_t)batch * stages.bb_r > SLOT_OUT_MAX)    /* the slots' pinned output buffers */
        batch = (int)(SLOT_OUT_MAX / stages.bb_r) > 0 ? (int)(SLOT_OUT_MAX / stages.bb_r) : 1;
    /* the handle may have produced blocks already (an earlier run or seek): the run continues
       from there; blocks before first_block are planned (the carrier chain) and dropped */
    if (first_block < info.next_block)
        return gss_fail(GSS_E_STATE, "run from block %lld, but the scenario is at block %lld",
                        (long long)first_block, (long long)info.next_block);

    /* the modes, then the run's context */
    Run r(run_modes_resolve(run_env_read(), opts && opts->carr_in, opts && opts->carr_predict,
                            info.carrier_int != 0, batch));
    r.stages = stages;
    r.scn = s;
    r.dev = d;
    r.opts = opts;
    r.carrier_int = info.carrier_int;
    r.threads = threads > 0 ? threads : 1;
    r.n_per_blk = info.n_per_blk;
    r.batch = batch;
    r.first = first_block;
    r.last = n_blocks < 0 ? INT64_MAX : first_block + n_blocks;
    r.start = info.next_block;
    RUN_TRY(hipGetDevice(&r.ordinal));

    int err = set_up(r, info, t_enter);
    if (err) {
        tear_down(r);
        return err;
    }
    if (trace_on())
        fprintf(stderr, "trace setup enter %.6f ready %.6f\n", t_enter, tnow());

    /* the threads; the walk kernels warmed while the planner produces its first rows */
    const int ordinal = r.ordinal;
    std::thread th([&r, ordinal] {
        (void)hipSetDevice(ordinal);                   /* pinned reallocations */
        planner(&r);
    });
    std::thread th_rows, th_prove;
    if (r.m.rows_ahead)
        th_rows = std::thread(rows_thread, &r);
    if (r.m.prover)
        th_prove = std::thread(prover, &r);
    if (r.m.spec)
        warm_walks(r);

    err = run_main(r, sink, user);

    post(r, r.abort, 1);
    th.join();
    if (th_rows.joinable())
        th_rows.join();
    if (th_prove.joinable())
        th_prove.join();
    if (r.m.rows_ahead && !err)                        /* the scenario's carriers: run's end */
        err = gss_scn_set_carrier(s, r.carr);
    tear_down(r);
    return err;
}

}  // namespace
}  // namespace gss_run_

extern "C" int gss_run(gss_dev *d, gss_scn *s, int64_t first_block, int64_t n_blocks, int batch,
                       int threads, gss_sink_fn sink, void *user)
{
    return gss_run_ex(d, s, first_block, n_blocks, batch, threads, sink, user, nullptr);
}

extern "C" int gss_run_ex(gss_dev *d, gss_scn *s, int64_t first_block, int64_t n_blocks,
                          int batch, int threads, gss_sink_fn sink, void *user,
                          const gss_run_opts_t *opts)
{
    using namespace gss_run_;
    if (!d || !s || !sink || first_block < 0)
        return gss_fail(GSS_E_ARG, "invalid run arguments");
    const double t_enter = trace_on() ? tnow() : 0.0;
    gss_scn_info_t info;
    int rc = gss_scn_info(s, &info);
    if (rc) return rc;
    const StageLaunches have = {gss_impair_device != nullptr, gss_jam_device != nullptr,
                                gss_echo_device != nullptr, gss_fir_device != nullptr};
    RunStages stages;
    rc = run_stages_resolve(opts, info, first_block, n_blocks, have, &stages);
    if (rc) return rc;
    /* a filtered range also renders the lead blocks that hold the filter's memory, and a
       wrapping sink keeps them from the caller's */
    const int64_t lead = stages.lead_blocks;
    TrimSink trim = {sink, user, first_block, stages.bb};
    return run_range(d, s, first_block - lead, n_blocks < 0 ? n_blocks : n_blocks + lead, batch,
                     threads, lead > 0 ? trim_sink : sink, lead > 0 ? (void *)&trim : user, opts,
                     info, stages, t_enter);
}

/* A plain C++ build (a CPU harness against a stand-in of the HIP runtime) that names this file
   alone still gets the whole driver: the other two translation units are taken in here.  A
   harness that compiles them itself, as the library's build always does, says so with
   GSS_RUN_SEPARATE (tests/fake_build.py, tools/sanitize.sh). */
#if !defined(__HIP__) && !defined(GSS_RUN_SEPARATE)
#include "gss_run_plan.hip"
#include "gss_run_pool.hip"
#endif
