/*
 * carr_chain.c — the carrier-phase chain the sample loop carries across blocks
 * (gpssim.c:2245-2250), over rows whose scenario is done with them.
 *
 * One chain per channel slot; a slot's chain restarts whenever allocateChannel re-initialises
 * its carr_phase.  Slots are independent, so every chain here runs one slot per pool part.
 *
 *   gss_carr_chain            the exact chain (every block walked, checkpoints on request)
 *   gss_carr_chain_starts/_guess, gss_carr_line_end, gss_spec_host
 *                             the block walks run ahead from guessed starts (gss_phase.h)
 *   gss_carr_chain_spec/_anchored, gss_carr_anchors
 *                             the chain from those walks, and its anchors
 *   gss_spec_links, gss_carr_chain_linked, gss_spec_records, gss_carr_chain_records
 *                             the walks folded into links and records, and the chains from them
 *
 * Nothing here knows a scenario (gss_scn): the rows, their counts and their gss_chain_t come from
 * gss_scn_next / gss_scn_next_deferred (scenario.c) or from the caller.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_phase.h"

/* The integer carrier (FLOAT_CARR_PHASE undefined): carr_phase += carr_phasestep per sample in
   a uint32 whose bits 16..24 index the LUT (gpssim.c:2202, 2252), i.e. a chain mod 2^25.  Rows
   carry it as multiples of 2^-25 cycle; n steps from x is (x + n step) mod 1, exactly. */
static double carr_int_walk(double x, double step, int n, double *ck)
{
    const uint32_t xi = (uint32_t)(x * K_CARR_INT_ONE);
    const int64_t si = (int64_t)(step * K_CARR_INT_ONE);
    if (ck)
        for (int j = 0; j < GSS_NCK; j++)
            ck[j] = (double)((xi + (uint32_t)(si * gss_ck_pos(j, n))) & 0x1FFFFFFu) /
                    K_CARR_INT_ONE;
    return (double)((xi + (uint32_t)(si * n)) & 0x1FFFFFFu) / K_CARR_INT_ONE;
}

double gss_carr_advance(double carr, double step, int64_t n)
{
    return gss_carr_walk_cc(carr, step, n);
}

double gss_carr_advance_ck(double carr, double step, int n, double *ck)
{
    return gss_carr_walk_ck(carr, step, n, ck);
}

/* Every call's argument rule: n and n_per_blk in range, the pointers the call always needs
   (always_ok) and those it needs once there are rows (rows_ok); `what` is the call's message. */
static int chain_args(int n, int n_per_blk, int always_ok, int rows_ok, const char *what)
{
    if (n < 0 || n_per_blk <= 0 || !always_ok || (n > 0 && !rows_ok))
        return gss_fail(GSS_E_ARG, "%s", what);
    return 0;
}

/* ---- the slot walk ----------------------------------------------------------------------------
 * One job for the whole chain family; a variant leaves the pointers it does not use NULL. */
typedef struct {
    double *carr;                       /* [K_MAX_CHAN] in: at the first block, out: after the last */
    gss_chan_blk_t *blk;                /* carr0 of every row written */
    const int32_t *nch;
    const gss_chain_t *chain;
    double *ck;
    const gss_spec_in_t *in;
    const gss_spec_t *spec;
    gss_carr_anchor_t *anch;
    const gss_spec_link_t *link;
    gss_spec_link_t *link_out;          /* gss_spec_links writes its records here */
    const gss_spec_rec_t *rec;
    int nblk, n_per_blk, carrier_int;
    int hits[K_MAX_CHAN];
} chain_job;

/* The rows of one channel slot in block order (a block holds at most one, among its first nch[b]
   <= GSS_MAXCH rows).  x is the slot's carrier at the current row's start: the walker replaces it
   with the row's end before it asks for the next row. */
typedef struct {
    int b;                              /* the next block to search */
    size_t e;                           /* the current row, b * GSS_MAXCH + k */
    int reset;                          /* the slot's chain restarted at the current row */
    double x;
} slot_it;

static inline slot_it slot_begin(const chain_job *j, int slot)
{
    const slot_it it = {0, 0, 0, j->carr ? j->carr[slot] : 0.0};
    return it;
}

/* the slot's next row (0: none left): a restart sets x to the row's init, and x is the row's
   carr0 where the job has rows to fill */
static inline int slot_next(const chain_job *j, int slot, slot_it *it)
{
    while (it->b < j->nblk) {
        const int b = it->b++;
        const int nk = j->nch[b] < GSS_MAXCH ? j->nch[b] : GSS_MAXCH;
        for (int k = 0; k < nk; k++) {
            const size_t e = (size_t)b * GSS_MAXCH + k;
            if (j->chain[e].slot != slot)
                continue;
            it->e = e;
            it->reset = j->chain[e].reset;
            if (it->reset)
                it->x = j->chain[e].init;
            if (j->blk)
                j->blk[e].carr0 = it->x;
            return 1;
        }
    }
    return 0;
}

/* one part per slot; the slots' summed hits into *n_hit (NULL: not wanted) */
static void chain_run(chain_job *j, gss_task_fn slot_part, int threads, int *n_hit)
{
    memset(j->hits, 0, sizeof j->hits);
    gss_pool_run(threads, K_MAX_CHAN, slot_part, j);
    if (n_hit == NULL)
        return;
    *n_hit = 0;
    for (int i = 0; i < K_MAX_CHAN; i++)
        *n_hit += j->hits[i];
}

/* ---- the exact chain ------------------------------------------------------------------------- */
static void plan_slot_part(void *arg, int slot)
{
    const chain_job *j = arg;
    slot_it it = slot_begin(j, slot);
    while (slot_next(j, slot, &it)) {
        const size_t e = it.e;
        if (j->carrier_int)        /* exact integer chain, checkpoints included */
            it.x = carr_int_walk(it.x, j->blk[e].carr_step, j->n_per_blk,
                                 j->ck ? j->ck + e * GSS_NCK : NULL);
        else if (j->ck) /* same walk, recording the sub-block checkpoints on the way */
            it.x = gss_carr_walk_ck(it.x, j->blk[e].carr_step, j->n_per_blk,
                                    j->ck + e * GSS_NCK);
        else
            it.x = gss_carr_walk_cc(it.x, j->blk[e].carr_step, j->n_per_blk);
    }
    j->carr[slot] = it.x;
}

/* The carrier chain (gpssim.c:2245-2250, carried across blocks) over nblk consecutive blocks:
   one chain per channel slot, restarted where allocateChannel re-initialised it; slots are
   independent, so one slot per thread. */
int gss_carr_chain(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                   const gss_chain_t *chain, int nblk, int n_per_blk, int carrier_int,
                   double *carr_ck, int threads)
{
    int rc = chain_args(nblk, n_per_blk, carr != NULL, blk && nch && chain,
                        "invalid carrier-chain arguments");
    if (rc)
        return rc;
    chain_job j = {.carr = carr, .blk = blk, .nch = nch, .chain = chain, .ck = carr_ck,
                   .nblk = nblk, .n_per_blk = n_per_blk, .carrier_int = carrier_int};
    chain_run(&j, plan_slot_part, threads, NULL);
    return 0;
}

/* ---- the chain with the block walks run ahead (gss_phase.h, speculative block walk) ---------- */
typedef struct {
    const gss_chan_blk_t *blk;
    int n_per_blk;
    gss_spec_in_t *in;
} guess_job;

static void guess_part(void *arg, int b)
{
    const guess_job *j = arg;
    for (int k = 0; k < GSS_MAXCH; k++) {
        gss_spec_in_t *r = &j->in[(size_t)b * GSS_MAXCH + k];
        if (r->k == 0)
            gss_spec_guess_row(r->g, r->s, j->n_per_blk, r);
    }
}

/* the starts, serially: the line of each slot from its exact start (in double: the drift over a
   batch, ~1e-13 per block, stays far inside the translation intervals); k = 0 on live rows (their
   segment starts not guessed yet), 1 on padding rows; pad = the index of the previous row of the
   same slot chain in the batch (-1: the slot's first row here, or a re-initialisation), which the
   records' links read (gss_spec_records*) */
static void chain_starts(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                         const gss_chain_t *chain, int nblk, int n_per_blk, gss_spec_in_t *in)
{
    double run[K_MAX_CHAN];
    int32_t last[K_MAX_CHAN];
    for (int i = 0; i < K_MAX_CHAN; i++) {
        run[i] = carr[i];
        last[i] = -1;
    }
    for (int b = 0; b < nblk; b++)
        for (int k = 0; k < GSS_MAXCH; k++) {
            const size_t e = (size_t)b * GSS_MAXCH + k;
            const int slot = k < nch[b] ? chain[e].slot : -1;
            in[e].k = 1;
            in[e].pad = -1;
            in[e].s = 0.0;
            in[e].g = 0.0;
            if (slot < 0 || slot >= K_MAX_CHAN)
                continue;
            if (chain[e].reset) {
                run[slot] = chain[e].init;
                last[slot] = -1;
            }
            in[e].pad = last[slot];
            last[slot] = (int32_t)e;
            const double g = run[slot];
            in[e].g = g >= 0.0 && g < 1.0 ? g : 0.0;
            in[e].s = blk[e].carr_step;
            in[e].k = 0;
            const double v = g + (double)n_per_blk * blk[e].carr_step;
            run[slot] = v - floor(v);
        }
}

/* The slots' carriers after the batch, predicted by the same lines (a start for the batch after
   it while its own chain is still pending: ~3e-10 cycle off after 2,048 blocks, far inside the
   translation intervals) */
int gss_carr_line_end(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                      const gss_chain_t *chain, int nblk, int n_per_blk, double *carr_end)
{
    int rc = chain_args(nblk, n_per_blk, carr && carr_end, blk && nch && chain,
                        "invalid carrier-line arguments");
    if (rc)
        return rc;
    double run[K_MAX_CHAN];
    for (int i = 0; i < K_MAX_CHAN; i++)
        run[i] = carr[i];
    for (int b = 0; b < nblk; b++)
        for (int k = 0; k < nch[b] && k < GSS_MAXCH; k++) {
            const size_t e = (size_t)b * GSS_MAXCH + k;
            const int slot = chain[e].slot;
            if (slot < 0 || slot >= K_MAX_CHAN)
                continue;
            if (chain[e].reset)
                run[slot] = chain[e].init;
            const double v = run[slot] + (double)n_per_blk * blk[e].carr_step;
            run[slot] = v - floor(v);
        }
    for (int i = 0; i < K_MAX_CHAN; i++)
        carr_end[i] = run[i];
    return 0;
}

int gss_carr_chain_starts(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                          const gss_chain_t *chain, int nblk, int n_per_blk, gss_spec_in_t *in)
{
    int rc = chain_args(nblk, n_per_blk, carr && in, blk && nch && chain,
                        "invalid carrier-guess arguments");
    if (rc)
        return rc;
    chain_starts(carr, blk, nch, chain, nblk, n_per_blk, in);
    return 0;
}

int gss_carr_chain_guess(const double *carr, const gss_chan_blk_t *blk, const int32_t *nch,
                         const gss_chain_t *chain, int nblk, int n_per_blk, gss_spec_in_t *in)
{
    int rc = gss_carr_chain_starts(carr, blk, nch, chain, nblk, n_per_blk, in);
    if (rc)
        return rc;
    /* the segment starts, in parallel over blocks */
    const guess_job j = {blk, n_per_blk, in};
    gss_pool_run(8, nblk, guess_part, (void *)&j);
    return 0;
}

typedef struct {
    gss_spec_in_t *in;
    int nrow, n_per_blk;
    gss_spec_t *spec;
} spec_host_job;

static void spec_host_part(void *arg, int part)
{
    const spec_host_job *j = arg;
    for (int i = part * 16; i < j->nrow && i < part * 16 + 16; i++) {
        if (j->in[i].k == 0)                     /* segment starts not guessed yet */
            gss_spec_guess_row(j->in[i].g, j->in[i].s, j->n_per_blk, &j->in[i]);
        for (int g = 0; g < j->in[i].k && g < GSS_SPEC_K; g++)
            gss_spec_seg_walk(&j->in[i], g, j->n_per_blk, &j->spec[i]);
    }
}

int gss_spec_host(gss_spec_in_t *in, int nrow, int n_per_blk, gss_spec_t *spec, int threads)
{
    int rc = chain_args(nrow, n_per_blk, 1, in && spec, "invalid speculative-walk arguments");
    if (rc)
        return rc;
    const spec_host_job j = {in, nrow, n_per_blk, spec};
    gss_pool_run(threads, (nrow + 15) / 16, spec_host_part, (void *)&j);
    return 0;
}

/* one row's end from its true start x; with a != NULL its anchors: the start, and the exact value
   at every segment start the fix-up passed or walked */
static double fix_row(double x, int n, const gss_spec_in_t *in, const gss_spec_t *o, int *hit,
                      double *d, gss_carr_anchor_t *a)
{
    if (a == NULL)
        return gss_spec_fix_d(x, n, in, o, hit, d, NULL);
    double av[GSS_SPEC_K];
    for (int j = 0; j < GSS_SPEC_K; j++)
        av[j] = -1.0;                                /* a carrier value is never negative */
    const double end = gss_spec_fix_d(x, n, in, o, hit, d, av);
    const int k = gss_spec_k(in);
    a->pos[0] = 0;
    a->val[0] = x;
    for (int j = 1; j < GSS_SPEC_K; j++) {
        const int ok = j < k && av[j] >= 0.0 && in->P[j] > 0 && in->P[j] < n;
        a->pos[j] = ok ? (int32_t)in->P[j] : -1;
        a->val[j] = ok ? av[j] : 0.0;
    }
    return end;
}

static void spec_slot_part(void *arg, int slot)
{
    chain_job *j = arg;
    slot_it it = slot_begin(j, slot);
    double d = 0.0;
    int hits = 0;
    while (slot_next(j, slot, &it)) {
        const size_t e = it.e;
        int hit = 0;
        it.x = fix_row(it.x, j->n_per_blk, &j->in[e], &j->spec[e], &hit, &d,
                       j->anch ? &j->anch[e] : NULL);
        hits += hit;
    }
    j->carr[slot] = it.x;
    j->hits[slot] = hits;
}

static void anchors_none(gss_carr_anchor_t *anch, int nblk)
{
    for (size_t e = 0; e < (size_t)nblk * GSS_MAXCH; e++)
        for (int j = 0; j < GSS_SPEC_K; j++) {
            anch[e].pos[j] = -1;
            anch[e].val[j] = 0.0;
        }
}

int gss_carr_chain_anchored(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                            const gss_chain_t *chain, int nblk, int n_per_blk,
                            const gss_spec_in_t *in, const gss_spec_t *spec, int threads,
                            int *n_hit, gss_carr_anchor_t *anch)
{
    int rc = chain_args(nblk, n_per_blk, carr != NULL, blk && nch && chain && in && spec,
                        "invalid carrier-chain arguments");
    if (rc)
        return rc;
    if (anch)
        anchors_none(anch, nblk);                     /* padding rows: none */
    chain_job j = {.carr = carr, .blk = blk, .nch = nch, .chain = chain, .in = in, .spec = spec,
                   .anch = anch, .nblk = nblk, .n_per_blk = n_per_blk};
    chain_run(&j, spec_slot_part, threads, n_hit);
    return 0;
}

int gss_carr_chain_spec(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                        const gss_chain_t *chain, int nblk, int n_per_blk,
                        const gss_spec_in_t *in, const gss_spec_t *spec, int threads,
                        int *n_hit)
{
    return gss_carr_chain_anchored(carr, blk, nch, chain, nblk, n_per_blk, in, spec, threads,
                                   n_hit, NULL);
}

/* anchors of rows whose carr0 the chain has set (any chain): in parallel over blocks */
typedef struct {
    const gss_chan_blk_t *blk;
    const int32_t *nch;
    const gss_spec_in_t *in;
    const gss_spec_t *spec;
    gss_carr_anchor_t *anch;
    int n_per_blk;
} anchor_job;

static void anchor_part(void *arg, int b)
{
    const anchor_job *j = arg;
    for (int k = 0; k < j->nch[b] && k < GSS_MAXCH; k++) {
        const size_t e = (size_t)b * GSS_MAXCH + k;
        gss_spec_anchors(j->blk[e].carr0, j->n_per_blk, &j->in[e], &j->spec[e],
                         j->anch[e].pos, j->anch[e].val);
    }
}

int gss_carr_anchors(const gss_chan_blk_t *blk, const int32_t *nch, int nblk, int n_per_blk,
                     const gss_spec_in_t *in, const gss_spec_t *spec, gss_carr_anchor_t *anch,
                     int threads)
{
    int rc = chain_args(nblk, n_per_blk, 1, blk && nch && in && spec && anch,
                        "invalid carrier-anchor arguments");
    if (rc)
        return rc;
    anchors_none(anch, nblk);
    const anchor_job j = {blk, nch, in, spec, anch, n_per_blk};
    gss_pool_run(threads, nblk, anchor_part, (void *)&j);
    return 0;
}

/* ---- links between a slot's consecutive rows (gss_spec_links / gss_carr_chain_linked) --------
 * Where row e' of a slot translated by d (its end = its last segment's end + d), the next row e of
 * the slot starts at y + d, y = that segment's end: known before the chain runs.  So e's partial
 * cycle to its first wrap is walked from y ahead of time with the admissible translations of y,
 * and e's whole walk folds into one record: e translates iff d is in [lo, hi], and then its own
 * last translation is d + dd and its end is end + (d + dd).  Exact: every translation the record
 * chains (d_0 = d + (w1' - w1), d_j+1 = d_j + (end_j - W_j+1)) is a sum of post-wrap lattice
 * values (multiples of 2^-52 ascending, 2^-53 descending, below 2 in magnitude), so the double
 * arithmetic carries it exactly, and the bounds lo_j - c_j are rounded inward. */
static void link_none(gss_spec_link_t *L)
{
    L->lo = 1.0;                                  /* an empty interval: no record */
    L->hi = 0.0;
    L->dd = L->end = 0.0;
}

/* the record of row e entered from y (the previous row's last segment end); 0: none, *L as it
   was */
static int link_row(double y, const gss_spec_in_t *in, const gss_spec_t *o, int64_t n,
                    gss_spec_link_t *L)
{
    double lo, hi, dd;
    if (!gss_spec_link_fold(y, in, o, n, &lo, &hi, &dd))
        return 0;
    L->lo = lo;
    L->hi = hi;
    L->dd = dd;
    L->end = o->seg[gss_spec_k(in) - 1].end;
    return 1;
}

/* every row's record is none on entry (gss_spec_links) */
static void link_slot_part(void *arg, int slot)
{
    const chain_job *j = arg;
    slot_it it = slot_begin(j, slot);
    int64_t prev = -1;
    while (slot_next(j, slot, &it)) {
        const size_t e = it.e;
        if (prev >= 0 && !it.reset && j->in[e].s != 0.0 && j->in[prev].s != 0.0)
            (void)link_row(j->spec[prev].seg[gss_spec_k(&j->in[prev]) - 1].end, &j->in[e],
                           &j->spec[e], j->n_per_blk, &j->link_out[e]);
        prev = (int64_t)e;
    }
}

int gss_spec_links(const int32_t *nch, const gss_chain_t *chain, int nblk, int n_per_blk,
                   const gss_spec_in_t *in, const gss_spec_t *spec, gss_spec_link_t *link,
                   int threads)
{
    int rc = chain_args(nblk, n_per_blk, 1, nch && chain && in && spec && link,
                        "invalid spec-link arguments");
    if (rc)
        return rc;
    for (size_t e = 0; e < (size_t)nblk * GSS_MAXCH; e++)
        link_none(&link[e]);
    chain_job j = {.nch = nch, .chain = chain, .in = in, .spec = spec, .link_out = link,
                   .nblk = nblk, .n_per_blk = n_per_blk};
    chain_run(&j, link_slot_part, threads, NULL);
    return 0;
}

static void linked_slot_part(void *arg, int slot)
{
    chain_job *j = arg;
    slot_it it = slot_begin(j, slot);
    double d = 0.0;
    int hits = 0, held = 0;
    while (slot_next(j, slot, &it)) {
        const size_t e = it.e;
        if (it.reset)
            held = 0;
        const gss_spec_link_t *L = &j->link[e];
        int hit = 0;
        if (held && d >= L->lo && d <= L->hi) {
            d += L->dd;
            it.x = L->end + d;
            hit = 1;
        } else {
            it.x = gss_spec_fix_d(it.x, j->n_per_blk, &j->in[e], &j->spec[e], &hit, &d, NULL);
        }
        held = hit;
        hits += hit;
    }
    j->carr[slot] = it.x;
    j->hits[slot] = hits;
}

int gss_carr_chain_linked(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                          const gss_chain_t *chain, int nblk, int n_per_blk,
                          const gss_spec_in_t *in, const gss_spec_t *spec,
                          const gss_spec_link_t *link, int threads, int *n_hit)
{
    int rc = chain_args(nblk, n_per_blk, carr != NULL,
                        blk && nch && chain && in && spec && link,
                        "invalid carrier-chain arguments");
    if (rc)
        return rc;
    chain_job j = {.carr = carr, .blk = blk, .nch = nch, .chain = chain, .in = in, .spec = spec,
                   .link = link, .nblk = nblk, .n_per_blk = n_per_blk};
    chain_run(&j, linked_slot_part, threads, n_hit);
    return 0;
}

/* ---- records: each row's walk folded (gss_phase.h gss_spec_record), the chain from them ------- */
typedef struct {
    const gss_spec_in_t *in;
    const gss_spec_t *spec;
    gss_spec_rec_t *rec;
    int nrow, n_per_blk;
} rec_job;

static void rec_part(void *arg, int part)
{
    const rec_job *j = arg;
    for (int i = part * 64; i < j->nrow && i < part * 64 + 64; i++) {
        const int p = j->in[i].pad;
        const int ok = p >= 0 && p < i;
        gss_spec_record(&j->in[i], &j->spec[i], ok ? &j->in[p] : NULL, ok ? &j->spec[p] : NULL,
                        j->n_per_blk, &j->rec[i]);
        if (j->rec[i].ok & 2)
            j->rec[i].ok |= (i - p) << 2;            /* the row the link was built against */
    }
}

int gss_spec_records(const gss_spec_in_t *in, const gss_spec_t *spec, int nrow, int n_per_blk,
                     gss_spec_rec_t *rec, int threads)
{
    int rc = chain_args(nrow, n_per_blk, 1, in && spec && rec, "invalid spec-record arguments");
    if (rc)
        return rc;
    const rec_job j = {in, spec, rec, nrow, n_per_blk};
    gss_pool_run(threads, (nrow + 63) / 64, rec_part, (void *)&j);
    return 0;
}

static void rec_slot_part(void *arg, int slot)
{
    chain_job *j = arg;
    const int64_t n = j->n_per_blk;
    slot_it it = slot_begin(j, slot);
    double d = 0.0;
    int hits = 0, held = 0;
    size_t e_prev = 0;                               /* the slot's previous row (held: valid) */
    while (slot_next(j, slot, &it)) {
        const size_t e = it.e;
        if (it.reset)
            held = 0;
        const gss_spec_rec_t *R = &j->rec[e];
        /* a link record holds only if it was built against this slot's previous row
           (ok bits 2.., the row distance; rows from elsewhere, e.g. zero-filled pads, fail
           the check and walk) */
        const int linked = held && (R->ok & 2) && (size_t)(R->ok >> 2) == e - e_prev;
        e_prev = e;
        if (linked && d >= R->llo && d <= R->lhi) {
            d += R->ldd;                             /* the link: no walk at all */
            it.x = R->end + d;
            hits++;
            continue;
        }
        const double s = j->blk[e].carr_step;
        double v = it.x;
        int wr = 0;
        const int64_t t = gss_carr_to_wrap(&v, s, n, &wr);
        held = 0;
        if (!wr || t >= n) {
            it.x = v;                                /* no wrap: walked exactly */
        } else if ((R->ok & 1) && t == R->p1 && v - R->w1 >= R->slo && v - R->w1 <= R->shi) {
            d = (v - R->w1) + R->sdd;                /* the row's own record */
            it.x = R->end + d;
            held = 1;
            hits++;
        } else {
            it.x = gss_carr_walk_cc(v, s, n - t);    /* a translation fails: the exact walk */
        }
    }
    j->carr[slot] = it.x;
    j->hits[slot] = hits;
}

int gss_carr_chain_records(double *carr, gss_chan_blk_t *blk, const int32_t *nch,
                           const gss_chain_t *chain, int nblk, int n_per_blk,
                           const gss_spec_rec_t *rec, int threads, int *n_hit)
{
    int rc = chain_args(nblk, n_per_blk, carr != NULL, blk && nch && chain && rec,
                        "invalid carrier-chain arguments");
    if (rc)
        return rc;
    chain_job j = {.carr = carr, .blk = blk, .nch = nch, .chain = chain, .rec = rec,
                   .nblk = nblk, .n_per_blk = n_per_blk};
    chain_run(&j, rec_slot_part, threads, n_hit);
    return 0;
}
