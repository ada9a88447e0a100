/*
 * gss_run_stages.h — the post-render stages of a streaming run (gss_run.hip: stages_apply),
 * resolved once at its start from the run's options by a pure function: what each stage was
 * given, the formats and block sizes that follow, and every refusal.  The chain, in order:
 *   echoes -> (jammers | impairment) -> filter
 * Plain C++17, no HIP: tests/helpers/run_stages_check.cpp compiles it with the host plane alone.
 */
#ifndef GSS_RUN_STAGES_H
#define GSS_RUN_STAGES_H
#include <stddef.h>
#include <stdint.h>
#include "gpssim_amd.h"

extern "C" int gss_fail(int code, const char *fmt, ...);
extern "C" int gss_jam_check(const gss_jam_t *jam, int n_jam);       /* jam.c */
extern "C" int gss_echo_check(const gss_echo_t *echo, int n_echo);   /* echo.c */
extern "C" int gss_fir_check(const gss_fir_t *fir);                  /* fir.c */

/* the stages' launches this build links (gss_run.hip fills it from its weak references) */
struct StageLaunches {
    bool impair, jam, echo, fir;
};

/* the run's copy of its stage options, and what follows from them */
struct RunStages {
    const gss_impair_t *impair = nullptr;   /* additive noise (opts->impair: the caller's, alive
                                               for the run), or null: no stage runs, the blocks
                                               render at the scenario's format */
    gss_jam_t jam[GSS_MAXJAM];              /* the run's copy of opts->jam */
    int n_jam = 0;
    gss_echo_t echo[GSS_MAXECHO];           /* the run's copy of opts->echo */
    int n_echo = 0;
    gss_fir_t fir;                          /* the front-end filter: the run's copy of opts->fir */
    bool has_fir = false;
    int fmt = 0;                     /* the format the blocks render at (SC16 with an impairment) */
    int fmt_out = 0;                 /* the scenario's format: what the sink receives          */
    size_t bb = 0, bb_r = 0;         /* bytes per block: to the sink, rendered                 */
    bool needs_imp_buf = false;      /* the last stage writes a second buffer per slot (d_imp):
                                        noise into SC08 / SC01, or any filtered run             */
    int64_t lead_blocks = 0;         /* blocks rendered before first_block for the filter's memory
                                        alone and kept from the caller's sink; 0 without a filter */
};

/* The filter's memory crosses every slot boundary, so a filtered run renders whole slots in run
   order and each block exactly once: it waits for each slot's GPU proof (submit_proven: no late
   verdicts, GSS_RUN_LATE_VERDICTS included) and never renders a block again (redo_rejected). */
static inline bool stages_need_order(const RunStages &g) { return g.has_fir; }

/* The stages of a run of blocks [first_block, first_block + n_blocks) (n_blocks < 0: to the end)
   of the scenario `info` describes; 0, or the refusal's code (gss_last_error has its text). */
static inline int run_stages_resolve(const gss_run_opts_t *opts, const gss_scn_info_t &info,
                                     int64_t first_block, int64_t n_blocks,
                                     const StageLaunches &have, RunStages *out)
{
    RunStages g{};
    int rc;
    g.fmt_out = info.data_format;
    g.bb = gss_block_bytes(info.n_per_blk, info.data_format);
    if (g.bb == 0)
        return gss_fail(GSS_E_ARG, "invalid format %d for %d samples/block", info.data_format,
                        info.n_per_blk);
    /* additive noise: the blocks render at SC16 (fmt, bb_r) and the impairment writes the
       scenario's format (bb bytes per block: what the sink receives) */
    const gss_impair_t *imp = opts ? opts->impair : nullptr;
    if (imp && (imp->sigma_q8 > 0x00FFFFFFu || imp->shift < 0 || imp->shift > 8))
        return gss_fail(GSS_E_ARG, "invalid impairment (sigma_q8 <= 0xFFFFFF, shift 0..8)");
    if (imp && !have.impair)
        return gss_fail(GSS_E_STATE, "additive noise requested, but this build has no "
                                     "impairment launch (gss_impair_device)");
    g.impair = imp;
    g.fmt = imp ? GSS_FMT_SC16 : info.data_format;
    g.bb_r = imp ? (size_t)info.n_per_blk * 4 : g.bb;
    g.n_jam = opts ? opts->n_jam : 0;
    if (g.n_jam < 0 || g.n_jam > GSS_MAXJAM || (g.n_jam > 0 && (!imp || !opts->jam)))
        return gss_fail(GSS_E_ARG, "invalid jammers (0..%d of them, with an impairment for "
                                   "the shift)", GSS_MAXJAM);
    if (g.n_jam > 0 && (rc = gss_jam_check(opts->jam, g.n_jam)) != 0)
        return rc;
    if (g.n_jam > 0 && !have.jam)
        return gss_fail(GSS_E_STATE, "jammers requested, but this build has no jammer launch "
                                     "(gss_jam_device)");
    for (int i = 0; i < g.n_jam; i++)
        g.jam[i] = opts->jam[i];
    g.n_echo = opts ? opts->n_echo : 0;
    if (g.n_echo < 0 || g.n_echo > GSS_MAXECHO || (g.n_echo > 0 && (!imp || !opts->echo)))
        return gss_fail(GSS_E_ARG, "invalid echoes (0..%d of them, with an impairment for the "
                                   "shift)", GSS_MAXECHO);
    if (g.n_echo > 0 && (rc = gss_echo_check(opts->echo, g.n_echo)) != 0)
        return rc;
    if (g.n_echo > 0 && !have.echo)
        return gss_fail(GSS_E_STATE, "echoes requested, but this build has no echo launch "
                                     "(gss_echo_device)");
    for (int i = 0; i < g.n_echo; i++)
        g.echo[i] = opts->echo[i];
    const gss_fir_t *fir = opts ? opts->fir : nullptr;
    if (fir && (!imp || opts->carr_in))
        return gss_fail(GSS_E_ARG, "the filter needs an impairment (sigma_q8 = 0: none) and no "
                                   "carrier hand-off (carr_in)");
    if (fir && (rc = gss_fir_check(fir)) != 0)
        return rc;
    if (fir && !have.fir)
        return gss_fail(GSS_E_STATE, "a filter requested, but this build has no filter launch "
                                     "(gss_fir_device)");
    g.has_fir = fir != nullptr;
    if (fir)
        g.fir = *fir;
    g.needs_imp_buf = imp && (g.fmt != g.fmt_out || g.has_fir);
    /* the filter's memory: a range that starts after block 0 also renders the blocks that hold
       the n_taps - 1 samples before it (one block, unless a block is shorter than that), so its
       bytes are the whole run's (an empty range renders nothing more than it did) */
    if (fir && first_block > 0 && fir->n_taps > 1 && n_blocks != 0) {
        const int64_t lead = ((int64_t)fir->n_taps - 2) / info.n_per_blk + 1;
        g.lead_blocks = lead > first_block ? first_block : lead;
        if (first_block - g.lead_blocks < info.next_block)
            return gss_fail(GSS_E_STATE, "a filtered run from block %lld needs block %lld, but the "
                            "scenario is at block %lld", (long long)first_block,
                            (long long)(first_block - g.lead_blocks), (long long)info.next_block);
    }
    *out = g;
    return 0;
}

#endif
