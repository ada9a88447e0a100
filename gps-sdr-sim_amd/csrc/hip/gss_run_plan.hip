/*
 * gss_run_plan.hip — the planning side of the streaming driver (gss_run.hip has the overview):
 * everything that runs on the planner, rows or prover thread.  A slot is theirs from FREE until
 * they post it PLANNED; the main thread (gss_run.hip) has it from then until it posts it FREE.
 *   rows_thread   the scenario's rows a batch ahead (r.m.rows_ahead)
 *   planner       per slot: its rows (plan_into: the chain run ahead, the up-front range of a
 *                 carrier hand-off, or the host chain), its nav sources, its host proof or its
 *                 GPU proof run ahead (proof_ahead)
 *   prover        the host proofs in slot order (r.m.prover)
 * Host code only: no kernel here.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "gss_run_impl.h"

namespace gss_run_ {
namespace {

/* The host proof of a slot (planner or prover thread): its certified lines and verdicts against
   the nav table (nav, n_nav rows), the exact-path list, its checkpoints.  force_exact is applied
   here only: the GPU proof takes it as an argument (proof_ahead). */
int prove_host(const Run &r, Slot &sl, const uint32_t *nav, int n_nav)
{
    const int rc = gss_linearize_ex(sl.blk, sl.nch, sl.nb, r.n_per_blk, r.ca, 32, nav, n_nav,
                                    sl.has_anch ? sl.anch : nullptr, sl.lin, sl.fast, r.threads);
    if (rc)
        return rc;
    if (r.m.force_exact > 0)
        for (int i = 0; i < sl.nb; i++)
            if ((sl.first + i) % r.m.force_exact == 0)
                sl.fast[i] = 0;
    list_exact(sl);
    fill_lazy_ck(r, sl);
    return 0;
}

/* the most channels of any of nb blocks (at least 1) */
int nch_max_of(const int32_t *nch, int nb)
{
    int m = 1;
    for (int i = 0; i < nb; i++)
        m = nch[i] > m ? nch[i] : m;
    return m;
}

/* The up-front range's chain run ahead on the GPU, in chunks of 4,096 blocks: each chunk's
   guesses from the exact carriers at its start, its walks, then its chain (exact). */
int chain_upfront_spec(Run &r, double *carr, const gss_chain_t *chain)
{
    constexpr int CH = 4096;
    const size_t rows_max = (size_t)CH * GSS_MAXCH;
    gss_spec_in_t *h_in = nullptr;                     /* pinned: the lanes use them directly */
    gss_spec_t *h_spec = nullptr;
    int rc = 0;
    if (pin_alloc((void **)&h_in, sizeof(gss_spec_in_t) * rows_max) !=
            hipSuccess ||
        pin_alloc((void **)&h_spec, sizeof(gss_spec_t) * rows_max) !=
            hipSuccess)
        rc = gss_fail(GSS_E_NOMEM, "carrier-chain buffers (%zu rows)", rows_max);
    int64_t hits = 0, n_rows = 0;
    for (int64_t b0 = 0; !rc && b0 < r.pre_n; b0 += CH) {
        const int nb = r.pre_n - b0 < CH ? (int)(r.pre_n - b0) : CH;
        const int nrow = nb * GSS_MAXCH;
        gss_chan_blk_t *blk = &r.pre_blk[(size_t)b0 * GSS_MAXCH];
        const int32_t *nch = &r.pre_nch[(size_t)b0];
        const gss_chain_t *ch = chain + (size_t)b0 * GSS_MAXCH;
        rc = gss_carr_chain_starts(carr, blk, nch, ch, nb, r.n_per_blk, h_in);
        if (rc) break;
        if ((rc = gss_spec_device(r.dev, h_in, nrow, r.n_per_blk, h_spec, r.spec_st)) != 0 ||
            hipStreamSynchronize(r.spec_st) != hipSuccess) {
            if (!rc) rc = gss_fail(GSS_E_HIP, "carrier-chain walks");
            break;
        }
        int hit = 0;
        rc = gss_carr_chain_spec(carr, blk, nch, ch, nb, r.n_per_blk, h_in, h_spec, r.threads,
                                 &hit);
        hits += hit;
        for (int i = 0; i < nb; i++)
            n_rows += nch[i];
    }
    if (trace_on())
        fprintf(stderr, "trace spec upfront rows %lld hits %lld\n", (long long)n_rows,
                (long long)hits);
    pin_free(h_in); pin_free(h_spec);
    return rc;
}

/* The walks' records of every row of the up-front range, CH blocks per launch, from starts per
   row (g: [pre_n][GSS_MAXCH]) or, without them, from the lines out of carr (the first pass) */
int upfront_records(Run &r, const gss_chain_t *chain, const double *carr, const double *g,
                    std::vector<gss_spec_rec_t> &rec)
{
    constexpr int CH = 4096;
    const size_t rows_max = (size_t)CH * GSS_MAXCH;
    gss_spec_in_t *h_in = nullptr, *d_in = nullptr;
    gss_spec_t *d_spec = nullptr;
    gss_spec_rec_t *h_rec = nullptr;
    int rc = 0;
    if (pin_alloc((void **)&h_in, sizeof(gss_spec_in_t) * rows_max) != hipSuccess ||
        pin_alloc((void **)&h_rec, sizeof(gss_spec_rec_t) * rows_max) != hipSuccess ||
        dev_alloc((void **)&d_in, sizeof(gss_spec_in_t) * rows_max) != hipSuccess ||
        dev_alloc((void **)&d_spec, sizeof(gss_spec_t) * rows_max) != hipSuccess)
        rc = gss_fail(GSS_E_NOMEM, "carrier-chain buffers (%zu rows)", rows_max);
    rec.resize((size_t)r.pre_n * GSS_MAXCH);
    double c[GSS_MAXCH];
    memcpy(c, carr, sizeof c);
    for (int64_t b0 = 0; !rc && b0 < r.pre_n; b0 += CH) {
        const int nb = r.pre_n - b0 < CH ? (int)(r.pre_n - b0) : CH;
        const int nrow = nb * GSS_MAXCH;
        const gss_chan_blk_t *blk = &r.pre_blk[(size_t)b0 * GSS_MAXCH];
        const int32_t *nch = &r.pre_nch[(size_t)b0];
        const gss_chain_t *ch = chain + (size_t)b0 * GSS_MAXCH;
        rc = gss_carr_chain_starts(c, blk, nch, ch, nb, r.n_per_blk, h_in);   /* k, s, pad */
        if (rc) break;
        if (g) {                                       /* the given starts instead of lines */
            for (int i = 0; i < nrow; i++)
                if (h_in[i].k == 0)
                    h_in[i].g = g[(size_t)b0 * GSS_MAXCH + i];
        } else {
            (void)gss_carr_line_end(c, blk, nch, ch, nb, r.n_per_blk, c);
        }
        if ((rc = gss_spec_records_device(r.dev, h_in, nrow, r.n_per_blk, d_in, d_spec, h_rec,
                                          r.spec_st)) != 0 ||
            hipStreamSynchronize(r.spec_st) != hipSuccess) {
            if (!rc) rc = gss_fail(GSS_E_HIP, "carrier-chain records");
            break;
        }
        memcpy(&rec[(size_t)b0 * GSS_MAXCH], h_rec, sizeof(gss_spec_rec_t) * (size_t)nrow);
    }
    pin_free(h_in); pin_free(h_rec); dev_free(d_in); dev_free(d_spec);
    return rc;
}

/* The up-front chain speculated across ranks (opts->carr_predict; shard.chain_speculated's
   steps): the range's map by the lines -> a predicted start -> walks and records from it -> the
   exact chain from that start and its map -> a second, ~1e-13 prediction -> the rows whose
   carrier depends on the start walked again from the first chain's carriers moved by the
   correction -> carr_in -> the records' chain (a compare and two adds per row where the
   links hold) -> carr_out.  Exact whatever the predictions. */
int chain_upfront_speculated(Run &r, const gss_chain_t *chain, const double *start0,
                             double *carr)
{
    const int64_t nb = r.pre_n;
    const size_t rows = (size_t)nb * GSS_MAXCH;
    const double t0 = tnow();
    int reset[GSS_MAXCH] = {0};
    for (int64_t b = 0; b < nb; b++)
        for (int k = 0; k < r.pre_nch[(size_t)b] && k < GSS_MAXCH; k++) {
            const gss_chain_t &c = chain[(size_t)b * GSS_MAXCH + k];
            if (c.reset && c.slot >= 0 && c.slot < GSS_MAXCH)
                reset[c.slot] = 1;
        }
    const bool exact0 = r.first == 0;                   /* the run's own start: no prediction */
    double zero[GSS_MAXCH] = {0}, end[GSS_MAXCH], map[3 * GSS_MAXCH], x0[GSS_MAXCH],
        x1[GSS_MAXCH];
    int rc = gss_carr_line_end(zero, r.pre_blk.data(), r.pre_nch.data(), chain, (int)nb,
                               r.n_per_blk, end);
    auto make_map = [&](const double *from, const double *to) {
        for (int i = 0; i < GSS_MAXCH; i++) {
            map[i] = exact0 ? start0[i] : 0.0;
            const double a = to[i] - from[i];
            map[GSS_MAXCH + i] = reset[i] ? to[i] : a - floor(a);
            map[2 * GSS_MAXCH + i] = reset[i] ? 1.0 : 0.0;
        }
    };
    make_map(zero, end);
    if (!rc && r.opts->carr_predict(r.opts->carr_user, 0, map, x0))
        rc = gss_fail(GSS_E_IO, "carrier prediction (round 0) failed at block %lld",
                      (long long)r.first);
    if (rc)
        return rc;
    if (exact0)
        memcpy(x0, start0, sizeof x0);
    std::vector<gss_spec_rec_t> rec;
    rc = upfront_records(r, chain, x0, nullptr, rec);
    if (rc)
        return rc;
    std::vector<gss_chan_blk_t> first(r.pre_blk);      /* the chain from the predicted start */
    double e0[GSS_MAXCH];
    memcpy(e0, x0, sizeof e0);
    int hit = 0;
    rc = gss_carr_chain_records(e0, first.data(), r.pre_nch.data(), chain, (int)nb, r.n_per_blk,
                                rec.data(), r.threads, &hit);
    if (rc)
        return rc;
    make_map(x0, e0);
    if (r.opts->carr_predict(r.opts->carr_user, 1, map, x1))
        return gss_fail(GSS_E_IO, "carrier prediction (round 1) failed at block %lld",
                        (long long)r.first);
    if (exact0)
        memcpy(x1, x0, sizeof x1);
    double d[GSS_MAXCH];
    bool moved = false;
    for (int i = 0; i < GSS_MAXCH; i++) {
        const double v = x1[i] - x0[i] + 0.5;
        d[i] = (v - floor(v)) - 0.5;
        moved = moved || (d[i] != 0.0 && !reset[i]);
    }
    int64_t rewalked = 0;
    if (moved) {                                       /* the start-dependent rows, corrected */
        std::vector<double> g(rows);
        int seen_reset[GSS_MAXCH] = {0};
        for (int64_t b = 0; b < nb; b++)
            for (int k = 0; k < GSS_MAXCH; k++) {
                const size_t e = (size_t)b * GSS_MAXCH + k;
                g[e] = first[e].carr0;
                if (k >= r.pre_nch[(size_t)b])
                    continue;
                const int sl = chain[e].slot;
                if (sl < 0 || sl >= GSS_MAXCH)
                    continue;
                if (chain[e].reset)
                    seen_reset[sl] = 1;
                if (!seen_reset[sl]) {
                    const double v = first[e].carr0 + d[sl];
                    g[e] = v - floor(v);
                    rewalked++;
                }
            }
        rc = upfront_records(r, chain, x1, g.data(), rec);
        if (rc)
            return rc;
    }
    const double t1 = tnow();
    if (r.opts->carr_in(r.opts->carr_user, carr))
        return gss_fail(GSS_E_IO, "carrier hand-off (in) failed at block %lld",
                        (long long)r.first);
    const double t2 = tnow();
    rc = gss_carr_chain_records(carr, r.pre_blk.data(), r.pre_nch.data(), chain, (int)nb,
                                r.n_per_blk, rec.data(), r.threads, &hit);
    if (trace_on())
        fprintf(stderr, "trace spec speculated rows %zu hits %d rewalked %lld pre %.6f wait %.6f "
                "handoff %.6f\n", rows, hit, (long long)rewalked, t1 - t0, t2 - t1, tnow() - t2);
    return rc;
}

/* gss_run_ex with a carrier hand-off: seek to the range, produce its rows, take the slot
   carriers at its first block from carr_in, walk the chain, give the end state to carr_out. */
int plan_range_upfront(Run &r)
{
    int rc = gss_scn_seek(r.scn, r.first, r.threads);
    if (rc)
        return rc;
    /* the speculated chain: with a prediction callback and the walks on the GPU */
    const bool speculate = r.opts->carr_predict && r.m.spec && r.m.rec;
    /* a prediction callback this rank will not use (GSS_RUN_SPEC=0, GSS_RUN_REC=0, the exact
       path): round -1 tells the ranks after it not to wait for its maps */
    if (r.opts->carr_predict && !speculate &&
        r.opts->carr_predict(r.opts->carr_user, -1, nullptr, nullptr))
        return gss_fail(GSS_E_IO, "carrier hand-off: publishing the no-speculation marker");
    double start0[GSS_MAXCH] = {0};
    if (speculate && r.first == 0 && (rc = gss_scn_carrier(r.scn, start0)) != 0)
        return rc;
    std::vector<gss_chain_t> chain;
    const int step = 4096;
    for (;;) {
        const int64_t want = r.last - r.first - r.pre_n;
        if (want <= 0)
            break;
        const int ask = want < step ? (int)want : step;
        r.pre_blk.resize((size_t)(r.pre_n + ask) * GSS_MAXCH);
        r.pre_nch.resize((size_t)(r.pre_n + ask));
        chain.resize((size_t)(r.pre_n + ask) * GSS_MAXCH);
        int nb = 0;
        rc = gss_scn_next_deferred(r.scn, ask, &r.pre_blk[(size_t)r.pre_n * GSS_MAXCH],
                                   &r.pre_nch[(size_t)r.pre_n],
                                   &chain[(size_t)r.pre_n * GSS_MAXCH], &nb, r.threads);
        if (rc)
            return rc;
        r.pre_n += nb;
        if (nb < ask)
            break;                                     /* end of the run */
    }
    double carr[GSS_MAXCH];
    if (!lazy_ck(r))
        r.pre_ck.resize((size_t)r.pre_n * GSS_MAXCH * GSS_NCK);
    if (speculate)                                     /* (takes carr_in itself, late) */
        rc = chain_upfront_speculated(r, chain.data(), start0, carr);
    else if (r.opts->carr_in(r.opts->carr_user, carr))
        return gss_fail(GSS_E_IO, "carrier hand-off (in) failed at block %lld",
                        (long long)r.first);
    else if (r.m.spec)                                 /* the chain run ahead on the GPU */
        rc = chain_upfront_spec(r, carr, chain.data());
    else
        rc = gss_carr_chain(carr, r.pre_blk.data(), r.pre_nch.data(), chain.data(),
                            (int)r.pre_n, r.n_per_blk, r.carrier_int,
                            lazy_ck(r) ? nullptr : r.pre_ck.data(), r.threads);
    if (rc)
        return rc;
    if (r.opts->carr_out && r.opts->carr_out(r.opts->carr_user, carr))
        return gss_fail(GSS_E_IO, "carrier hand-off (out) failed after block %lld",
                        (long long)(r.first + r.pre_n - 1));
    return 0;
}

/* The nav rows new since the previous slot, as sources for the GPU producer: rows
   [r.nav_planned, upto) of the scenario's table (rows are appended in run order). */
int take_nav_sources(Run &r, Slot &sl, int upto)
{
    const gss_nav_src_t *src = nullptr;
    int n_all = 0;
    if (r.m.rows_ahead) {
        src = r.nav_src_h.data();
        n_all = (int)r.nav_src_h.size();
    } else {
        gss_scn_nav_sources(r.scn, &src, &n_all);
    }
    if (upto > n_all)
        upto = n_all;
    const int n = upto > r.nav_planned ? upto - r.nav_planned : 0;
    if (n > sl.nav_cap) {
        pin_free(sl.nav);
        sl.nav = nullptr;
        sl.nav_cap = 0;
        const int cap = n * 2 + 16;
        if (pin_alloc((void **)&sl.nav, sizeof(gss_nav_src_t) * (size_t)cap) != hipSuccess)
            return gss_fail(GSS_E_NOMEM, "pinned nav sources");
        sl.nav_cap = cap;
    }
    if (n > 0)
        memcpy(sl.nav, src + r.nav_planned, sizeof(gss_nav_src_t) * (size_t)n);
    /* the chains' next links within the slot's rows, from their prev links: the rows thread's
       copies (nav_src_h) were taken when each row was new, before its successor existed, and
       gss_nav_kernel reaches every row but a chain's head through them */
    for (int i = 0; i < n; i++)
        sl.nav[i].next = -1;
    for (int i = 0; i < n; i++) {
        const int pv = sl.nav[i].prev;
        if (pv >= r.nav_planned && pv < r.nav_planned + i)
            sl.nav[pv - r.nav_planned].next = r.nav_planned + i;
    }
    sl.nav_first = r.nav_planned;
    sl.n_nav = n;
    r.nav_planned += n;
    return 0;
}

/* the slot's batch from the up-front plan (rows keep their global nav indices) */
int take_upfront(Run &r, Slot &sl, int *nb_out)
{
    const int64_t left = r.pre_n - r.pre_at;
    const int nb = left < r.batch ? (int)left : r.batch;
    *nb_out = nb;
    if (nb <= 0)
        return 0;
    const size_t rows = (size_t)nb * GSS_MAXCH;
    memcpy(sl.blk, &r.pre_blk[(size_t)r.pre_at * GSS_MAXCH], rows * sizeof(gss_chan_blk_t));
    memcpy(sl.nch, &r.pre_nch[(size_t)r.pre_at], (size_t)nb * sizeof(int32_t));
    if (!lazy_ck(r))
        memcpy(sl.ck, &r.pre_ck[(size_t)r.pre_at * GSS_MAXCH * GSS_NCK],
               rows * GSS_NCK * sizeof(double));
    int hi = -1;
    for (int b = 0; b < nb; b++)
        for (int k = 0; k < sl.nch[b]; k++) {
            const int t = sl.blk[(size_t)b * GSS_MAXCH + k].nav_tbl;
            hi = t > hi ? t : hi;
        }
    const int rc = take_nav_sources(r, sl, hi + 1);
    if (rc)
        return rc;
    sl.first = r.first + r.pre_at;
    r.pre_at += nb;
    return 0;
}

/* the next batch's size from the cursor: stops exactly at the range start and at its end */
int next_ask(const Run &r, int64_t cursor)
{
    const int64_t want = r.last - cursor;
    if (want <= 0)
        return 0;
    int ask = want < r.batch ? (int)want : r.batch;
    if (cursor < r.first && r.first - cursor < ask)
        ask = (int)(r.first - cursor);
    return ask;
}

/* The carrier chain run ahead on the GPU (gss_run.hip's header), in two steps per batch:
   spec_launch produces the batch's rows (carriers deferred) and its guesses and queues the GPU
   walks; spec_finish waits for them, walks the chain (exact) and hands the rows over.  The
   planner launches batch k+1 right after finishing batch k, so that k+1's walks run on the GPU
   while k's proofs run on the host. */

/* the next batch of rows_ahead into b (vectors swapped, no copy); its nav rows and sources onto
   the planner's copies */
int take_rows(Run &r, Run::SpecBatch &b, int *nb_out)
{
    *nb_out = 0;
    Run::RowBatch &q = r.rb[r.rb_take];
    const double tw = trace_on() ? tnow() : 0.0;
    {
        std::unique_lock<std::mutex> lk(r.mu);
        r.cv.wait(lk, [&] { return r.abort || q.ready || r.rows_done; });
        if (!q.ready)
            return gss_fail(GSS_E_STATE, r.abort ? "run aborted" : "rows ended before the run");
    }
    if (q.err)
        return q.err;
    std::swap(b.blk, q.blk);
    std::swap(b.nch, q.nch);
    std::swap(b.chain, q.chain);
    if (r.nav_rows_h.size() + q.nav_rows.size() > r.nav_rows_h.capacity()) {
        /* beyond the reservation (not expected): the prover reads the table, so grow it only
           with no slot in its hands */
        std::unique_lock<std::mutex> lk(r.mu);
        r.cv.wait(lk, [&] {
            for (const Slot &x : r.slot)
                if (x.state == PROVING)
                    return r.abort != 0;
            return true;
        });
        if (r.abort)
            return gss_fail(GSS_E_STATE, "run aborted");
    }
    r.nav_src_h.insert(r.nav_src_h.end(), q.nav_src.begin(), q.nav_src.end());
    r.nav_rows_h.insert(r.nav_rows_h.end(), q.nav_rows.begin(), q.nav_rows.end());
    *nb_out = q.nb;
    if (trace_on())
        fprintf(stderr, "trace rows nb %d produced %.6f %.6f wait %.6f\n", q.nb, q.t0, q.t1,
                tnow() - tw);
    post(r, q.ready, 0);
    r.rb_take ^= 1;
    return 0;
}

int spec_launch(Run &r, Run::SpecBatch &b, int ask)
{
    b.nb = 0;
    b.launched = 1;
    int rc = 0, nb = 0;
    if (r.m.rows_ahead) {
        /* the finished batches' exact carriers, carried by the lines through the batch still in
           flight (if any): a prediction, ~3e-10 cycle off, which only the guesses use */
        memcpy(b.carr, r.carr, sizeof b.carr);
        for (int f = 0; f < r.n_fly; f++) {
            const Run::SpecBatch &p = r.sb[(r.sb_head + f) % 3];
            if (p.nb > 0)
                (void)gss_carr_line_end(b.carr, p.blk.data(), p.nch.data(), p.chain.data(), p.nb,
                                        r.n_per_blk, b.carr);
        }
        rc = take_rows(r, b, &nb);
    } else {
        rc = gss_scn_carrier(r.scn, b.carr);
        if (!rc)
            rc = gss_scn_next_deferred(r.scn, ask, b.blk.data(), b.nch.data(), b.chain.data(),
                                       &nb, r.threads);
    }
    if (rc || nb == 0)
        return rc;
    b.nb = nb;
    const int nrow = nb * GSS_MAXCH;
    b.tg = trace_on() ? tnow() : 0.0;
    rc = gss_carr_chain_starts(b.carr, b.blk.data(), b.nch.data(), b.chain.data(), nb,
                               r.n_per_blk, b.h_in);           /* the walkers guess the rest */
    if (rc)
        return rc;
    /* the lanes read their rows from, and write their walks to, the pinned host buffers
       directly (a few hundred bytes each): no copy engine in the loop (it queues behind the
       slots' downloads).  Staging them through device memory by copy kernels (one pass of
       16-byte copies each way) measured the same: the downloads beside them run at ~0.8 of the
       link either way, the walks' own traffic (~14 MB per 2048-block slot back to the host,
       with the 10 MB of uploads) sharing its device-to-host direction */
    if (b.consumed_pending) {            /* a GPU proof still reads the batch's device walks */
        RUN_TRY(hipStreamWaitEvent(r.spec_st, b.consumed, 0));
        b.consumed_pending = 0;
    }
    rc = r.m.rec ? gss_spec_records_device(r.dev, b.h_in, nrow, r.n_per_blk, b.d_in, b.d_spec,
                                         b.h_rec, r.spec_st)
               : gss_spec_device(r.dev, b.h_in, nrow, r.n_per_blk, b.h_spec, r.spec_st);
    if (rc)
        return rc;
    RUN_TRY(hipEventRecord(b.walked, r.spec_st));    /* not the stream: later batches queue */
    b.tk = trace_on() ? tnow() : 0.0;
    return 0;
}

/* the batch's chain; anch (NULL: none): its anchors for the slot's proofs */
int spec_finish(Run &r, Run::SpecBatch &b, gss_chan_blk_t *blk, int32_t *nch, int *nb_out,
                gss_carr_anchor_t *anch)
{
    b.launched = 0;
    *nb_out = 0;
    const int nb = b.nb;
    b.nb = 0;
    if (nb == 0)
        return 0;
    const double tw = trace_on() ? tnow() : 0.0;
    RUN_TRY(hipEventSynchronize(b.walked));
    const double t0 = trace_on() ? tnow() : 0.0;
    double carr[GSS_MAXCH];                          /* exact: the batches before are done */
    memcpy(carr, r.m.rows_ahead ? r.carr : b.carr, sizeof carr);
    int hit = 0;
    int rc = r.m.rec ? gss_carr_chain_records(carr, b.blk.data(), b.nch.data(), b.chain.data(), nb,
                                            r.n_per_blk, b.h_rec, r.threads, &hit)
                   : gss_carr_chain_anchored(carr, b.blk.data(), b.nch.data(), b.chain.data(),
                                             nb, r.n_per_blk, b.h_in, b.h_spec, r.threads, &hit,
                                             anch);
    if (rc)
        return rc;
    if (r.m.rows_ahead)
        memcpy(r.carr, carr, sizeof carr);             /* the scenario is the rows thread's */
    else
        rc = gss_scn_set_carrier(r.scn, carr);
    if (rc)
        return rc;
    memcpy(blk, b.blk.data(), sizeof(gss_chan_blk_t) * GSS_MAXCH * (size_t)nb);
    memcpy(nch, b.nch.data(), sizeof(int32_t) * (size_t)nb);
    int rows = 0;
    for (int i = 0; i < nb; i++)
        rows += nch[i];
    r.spec_rows += rows;
    r.spec_hits += hit;
    if (trace_on())
        fprintf(stderr, "trace spec nb %d rows %d hits %d guess %.6f gpu_wait %.6f chain %.6f\n",
                nb, rows, hit, b.tk - b.tg, t0 - tw, tnow() - t0);
    *nb_out = nb;
    return 0;
}

/* Fill slot k's pinned buffers with the next batch inside [first, last); without a carrier
   hand-off, blocks before `first` are planned (the carrier chain is serial) and dropped. */
int plan_into(Run &r, Slot &sl, int64_t *cursor)
{
    sl.has_anch = 0;
    sl.sb_idx = -1;
    if (r.opts && r.opts->carr_in) {
        int nb = 0;
        int rc = take_upfront(r, sl, &nb);
        if (rc)
            return rc;
        if (nb == 0) {
            sl.nb = 0;
            sl.end = 1;
            return 0;
        }
        sl.nb = nb;
        sl.nch_max = nch_max_of(sl.nch, nb);
        sl.n_fb = 0;
        if (r.m.use_lin && !sl.gpu_proven) {
            const uint32_t *rows = nullptr;
            int n_rows = 0;
            gss_scn_nav_table(r.scn, &rows, &n_rows);
            return prove_host(r, sl, rows, n_rows);
        }
        return 0;
    }
    for (;;) {
        const int ask = next_ask(r, *cursor);
        int nb = 0;
        int rc = 0;
        if (r.m.rows_ahead) {
            /* two batches' walks in flight: the oldest is finished (its chain, exact) while the
               next one's walks run on the GPU; the batch after that is launched first */
            while (!rc && r.n_fly < 2 && !r.fly_end) {
                int64_t lc = *cursor;
                for (int f = 0; f < r.n_fly; f++)
                    lc += r.sb[(r.sb_head + f) % 3].nb;
                const int a = next_ask(r, lc);
                if (a <= 0)
                    break;
                Run::SpecBatch &b = r.sb[(r.sb_head + r.n_fly) % 3];
                rc = spec_launch(r, b, a);
                r.n_fly++;
                if (!rc && b.nb == 0)
                    r.fly_end = 1;                     /* the scenario's end */
            }
            if (!rc && r.n_fly > 0) {
                rc = spec_finish(r, r.sb[r.sb_head], sl.blk, sl.nch, &nb, sl.anch);
                sl.sb_idx = r.sb_head;
                r.sb_head = (r.sb_head + 1) % 3;
                r.n_fly--;
            }
        } else if (r.m.spec) {
            Run::SpecBatch &b = r.sb[r.sb_cur];
            if (!b.launched && ask > 0)
                rc = spec_launch(r, b, ask);
            if (!rc && b.launched) {                   /* else the range is done: nb stays 0 */
                rc = spec_finish(r, b, sl.blk, sl.nch, &nb, sl.anch);
                sl.sb_idx = r.sb_cur;                  /* the walks this slot's anchors are in */
            }
            if (!rc && nb > 0) {                       /* the next batch's walks, on the GPU now */
                const int ask2 = next_ask(r, *cursor + nb);
                r.sb_cur ^= 1;
                if (ask2 > 0)
                    rc = spec_launch(r, r.sb[r.sb_cur], ask2);
            }
        } else if (ask > 0) {
            /* before the range only the carrier chain matters: no checkpoints recorded */
            rc = gss_scn_next(r.scn, ask, sl.blk, sl.nch,
                              (*cursor < r.first || lazy_ck(r)) ? nullptr : sl.ck, &nb, r.threads);
        }
        if (rc)
            return rc;
        if (nb == 0) {
            sl.nb = 0;
            sl.end = 1;
            return 0;
        }
        int64_t b0 = *cursor;
        *cursor += nb;
        if (b0 < r.first)
            continue;                                  /* before the range: planned, dropped */
        sl.first = b0;
        sl.nb = nb;
        sl.has_anch = sl.anch != nullptr && r.m.spec && !r.m.rec;
        sl.nch_max = nch_max_of(sl.nch, nb);
        const uint32_t *rows = nullptr;
        int n_rows = 0;
        if (r.m.rows_ahead) {
            rows = r.nav_rows_h.data();
            n_rows = (int)(r.nav_rows_h.size() / GSS_NAV_WORDS);
        } else {
            gss_scn_nav_table(r.scn, &rows, &n_rows);
        }
        rc = take_nav_sources(r, sl, n_rows);          /* the GPU builds the new rows */
        if (rc)
            return rc;
        if (r.m.prover) {                                /* the proofs, on the prover thread */
            sl.lin_nav = rows;
            sl.lin_n_nav = n_rows;
            return 0;
        }
        sl.n_fb = 0;
        if (r.m.use_lin && !sl.gpu_proven) {             /* the proofs, on the planner thread */
            if (trace_on())
                fprintf(stderr, "trace scn_done %.6f\n", tnow());
            return prove_host(r, sl, rows, n_rows);
        }
        return 0;
    }
}

/* GPU proofs, run ahead (planner thread, right after the slot is planned): the slot's rows go
   to its device buffer on its own stream, its new nav rows are built on the planner's nav
   stream (in slot order: a row may continue the one before it), and the proof kernel runs as
   soon as both are there, so that several slots' proofs overlap the downloads of the slots
   before them instead of waiting on the render stream.  The device nav table was reserved for
   the whole run at set-up, so it never moves under the renders. */
int proof_ahead(Run &r, Slot &sl)
{
    /* the nav rows of every slot come from here when any slot is proven on the GPU (a row may
       continue one that an earlier slot brought); the proof only for the slots that take it */
    int rc = slot_in_reserve(sl, nullptr);             /* the slot is FREE: nothing reads it */
    if (rc)
        return rc;
    const SlotDev v = slot_dev(sl);
    const int n_rows = slot_nav_rows(sl);
    if ((size_t)n_rows > r.d_nav_cap)
        return gss_fail(GSS_E_RANGE, "nav rows %d past the run's reservation %zu", n_rows,
                        r.d_nav_cap);
    if (sl.n_nav > 0) {
        RUN_H2D(v.src, sl.nav, sizeof(gss_nav_src_t) * (size_t)sl.n_nav, r.nav_st);
        rc = gss_nav_rows_device(r.dev, v.src, sl.nav_first, sl.n_nav, r.d_nav, r.nav_st);
        if (rc)
            return rc;
    }
    RUN_TRY(hipEventRecord(sl.navd, r.nav_st));
    if (!sl.gpu_proven)
        return 0;
    RUN_H2D(v.blk, sl.blk, sizeof(gss_chan_blk_t) * GSS_MAXCH * (size_t)sl.nb, sl.pst);
    RUN_H2D(v.nch, sl.nch, sizeof(int32_t) * (size_t)sl.nb, sl.pst);
    if (!lazy_ck(r))               /* (with lazy checkpoints only a rejected block needs them) */
        RUN_H2D(v.ck, sl.ck, sizeof(double) * GSS_MAXCH * GSS_NCK * (size_t)sl.nb, sl.pst);
    if (v.anch)
        RUN_H2D(v.anch, sl.anch, sizeof(gss_carr_anchor_t) * GSS_MAXCH * (size_t)sl.nb, sl.pst);
    RUN_TRY(hipStreamWaitEvent(sl.pst, sl.navd, 0));
    Run::SpecBatch *sb = r.m.rec && r.m.dev_anch && sl.sb_idx >= 0 && !v.anch ? &r.sb[sl.sb_idx]
                                                                          : nullptr;
    rc = run_proof_launch(v.blk, v.nch, sl.nb, r.n_per_blk, r.d_ca, 32, r.d_nav, n_rows, v.anch,
                          sb ? sb->d_in : nullptr, sb ? sb->d_spec : nullptr, v.lin, v.fast,
                          sl.first, r.m.force_exact, sl.pst);
    if (rc)
        return rc;
    if (sb) {                                /* the batch's next walks wait for this proof */
        RUN_TRY(hipEventRecord(sb->consumed, sl.pst));
        sb->consumed_pending = 1;
    }
    /* the verdicts to the host at once: when the proof is done by the slot's submission, its
       rejected blocks take the exact path in the same render (submit_proven) */
    RUN_TRY(hipMemcpyAsync(sl.fast, v.fast, sizeof(int32_t) * (size_t)sl.nb,
                           hipMemcpyDeviceToHost, sl.pst));
    RUN_TRY(hipEventRecord(sl.proved, sl.pst));
    return 0;
}

}  // namespace

/* next_ask's batches in run order, produced ahead of the planner (rows_ahead): the scenario's
   rows with their carriers deferred, and the nav rows and sources new with each batch */
void rows_thread(Run *r)
{
    gss_pool_select(r->m.rows_pool ? 1 : 0);           /* 0: share the planner's workers */
    int64_t cursor = r->start;
    int nav_done = 0;
    for (int i = 0;; i++) {
        Run::RowBatch &q = r->rb[i & 1];
        {
            std::unique_lock<std::mutex> lk(r->mu);
            r->cv.wait(lk, [&] { return r->abort || !q.ready; });
            if (r->abort)
                break;
        }
        const int ask = next_ask(*r, cursor);
        if (ask <= 0)
            break;                                     /* the planner asks no further */
        q.t0 = trace_on() ? tnow() : 0.0;
        int nb = 0;
        int rc = gss_scn_next_deferred(r->scn, ask, q.blk.data(), q.nch.data(), q.chain.data(),
                                       &nb, r->threads);
        const gss_nav_src_t *src = nullptr;
        const uint32_t *rows = nullptr;
        int n_src = 0, n_rows = 0;
        if (!rc)
            rc = gss_scn_nav_sources(r->scn, &src, &n_src);
        if (!rc)
            rc = gss_scn_nav_table(r->scn, &rows, &n_rows);
        if (!rc && (n_src != n_rows || n_src < nav_done))
            rc = gss_fail(GSS_E_STATE, "nav table and sources out of step");
        if (!rc) {
            q.nav_src.assign(src + nav_done, src + n_src);
            q.nav_rows.assign(rows + (size_t)nav_done * GSS_NAV_WORDS,
                              rows + (size_t)n_rows * GSS_NAV_WORDS);
            nav_done = n_src;
        }
        q.first = cursor;
        q.nb = nb;
        q.err = rc;
        q.end = rc || nb == 0;
        cursor += nb;
        q.t1 = trace_on() ? tnow() : 0.0;
        post(*r, q.ready, 1);
        if (q.end)
            break;
    }
    post(*r, r->rows_done, 1);
}

void planner(Run *r)
{
    int64_t cursor = r->start;
    int up_rc = (r->opts && r->opts->carr_in) ? plan_range_upfront(*r) : 0;
    for (int i = 0;; i++) {
        Slot &sl = r->slot[i % NSLOT];
        {
            std::unique_lock<std::mutex> lk(r->mu);
            r->cv.wait(lk, [&] { return r->abort || sl.state == FREE; });
            if (r->abort)
                return;
        }
        const double t0 = trace_on() ? tnow() : 0.0;
        sl.gpu_proven = r->m.use_lin && (r->m.proof_mode == 1 || (r->m.proof_mode == 2 && (i & 1)));
        int rc = up_rc ? up_rc : plan_into(*r, sl, &cursor);
        if (!rc && !sl.end && r->m.gpu_proof)
            rc = proof_ahead(*r, sl);
        if (trace_on())
            fprintf(stderr, "trace plan slot %d nb %d %.6f %.6f\n", i % NSLOT, sl.nb, t0, tnow());
        {
            std::lock_guard<std::mutex> lk(r->mu);
            if (rc) {
                sl.err = rc;
                sl.end = 1;
            }
            sl.state = r->m.prover ? PROVING : PLANNED;
        }
        r->cv.notify_all();
        if (sl.end)
            return;
    }
}

/* The slots' proofs in slot order (r.m.prover): gss_linearize on this thread's own worker pool,
   the exact-path block list and its checkpoints, then the slot goes to the main thread. */
void prover(Run *r)
{
    gss_pool_select(2);
    for (int i = 0;; i++) {
        Slot &sl = r->slot[i % NSLOT];
        {
            std::unique_lock<std::mutex> lk(r->mu);
            r->cv.wait(lk, [&] { return r->abort || sl.state == PROVING; });
            if (r->abort)
                return;
        }
        const double t0 = trace_on() ? tnow() : 0.0;
        if (!sl.end && !sl.err && !sl.gpu_proven) {
            const int rc = prove_host(*r, sl, sl.lin_nav, sl.lin_n_nav);
            if (rc) {
                sl.err = rc;
                sl.end = 1;
            }
        }
        if (trace_on())
            fprintf(stderr, "trace prove slot %d nb %d %.6f %.6f\n", i % NSLOT, sl.nb, t0, tnow());
        const int end = sl.end;
        post(*r, sl.state, PLANNED);
        if (end)
            return;
    }
}

}  // namespace gss_run_
