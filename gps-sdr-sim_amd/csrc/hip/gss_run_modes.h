/*
 * gss_run_modes.h — the modes of a streaming run (gss_run.hip), resolved once at its start from
 * the environment switches (their table: gss_run.hip's header) and the run's arguments by a pure
 * function.  Plain C++17, no HIP: tests/helpers/run_modes_check.cpp compiles it alone.
 */
#ifndef GSS_RUN_MODES_H
#define GSS_RUN_MODES_H
#include <stdlib.h>
#include <string.h>

/* the switches as the environment holds them (NULL: unset); GSS_PATH, else GSS_RUN_<NAME> */
struct RunEnv {
    const char *path = nullptr, *force_exact = nullptr, *late_verdicts = nullptr;
    const char *upload = nullptr, *spec = nullptr, *rec = nullptr, *dev_anchors = nullptr;
    const char *anchors = nullptr, *rows_ahead = nullptr, *rows_pool = nullptr;
    const char *proof = nullptr, *prover = nullptr, *spec_cus = nullptr, *render_rest = nullptr;
};

/* every getenv of a run (GSS_RUN_TRACE apart: cached per process, gss_run_impl.h: trace_on) */
static inline RunEnv run_env_read()
{
    RunEnv e;
    e.path = getenv("GSS_PATH");
    e.force_exact = getenv("GSS_RUN_FORCE_EXACT");
    e.late_verdicts = getenv("GSS_RUN_LATE_VERDICTS");
    e.upload = getenv("GSS_RUN_UPLOAD");
    e.spec = getenv("GSS_RUN_SPEC");
    e.rec = getenv("GSS_RUN_REC");
    e.dev_anchors = getenv("GSS_RUN_DEV_ANCHORS");
    e.anchors = getenv("GSS_RUN_ANCHORS");
    e.rows_ahead = getenv("GSS_RUN_ROWS_AHEAD");
    e.rows_pool = getenv("GSS_RUN_ROWS_POOL");
    e.proof = getenv("GSS_RUN_PROOF");
    e.prover = getenv("GSS_RUN_PROVER");
    e.spec_cus = getenv("GSS_RUN_SPEC_CUS");
    e.render_rest = getenv("GSS_RUN_RENDER_REST");
    return e;
}

struct RunModes {
    int use_lin = 1;         /* the fast path (certified lines); 0: every block on the exact path */
    int force_exact = 0;     /* k > 0: every k-th block of the run to the exact path (tests) */
    int late_verdicts = 0;   /* tests: submit_proven takes every GPU proof as still running, so
                                rejected blocks always take the redo path in drain */
    int upload_dev = 1;      /* the slots' inputs uploaded by a copy kernel; 0: the copy engine */
    int spec = 0;            /* the carrier chain run ahead on the GPU: per batch (gss_run), or over
                                the up-front range (hand-off) */
    int rec = 0;             /* ... the walks' records, not the walks, back from the GPU */
    int dev_anch = 0;        /* records mode: GPU proofs anchored on the batch's device walks */
    int anchors = 0;         /* the slots hold the chain's anchors for the proofs' carrier walks
                                (filled, Slot::has_anch, only when the walks come back: !rec) */
    int rows_ahead = 0;      /* the rows produced ahead on their own thread */
    int rows_pool = 1;       /* ... on its own worker pool; 0: the planner's */
    int proof_mode = 0;      /* 0: host proofs, 1: all on the GPU, 2: every other slot */
    int gpu_proof = 0;       /* any proofs on the GPU, run ahead by the planner (proof_ahead) */
    int prover = 0;          /* host proofs on their own thread (slots handed over PROVING) */
    int spec_cus = 0;        /* N > 0 (measurement): the walks' stream on N of the device's CUs */
    int render_rest = 0;     /* ... and the render stream on the others */
};

/* has_carr_in / has_carr_predict: the run's carrier hand-off callbacks (gss_run_opts_t);
   clamped_batch: blocks per slot after the clamp to the slots' output buffers.  The order below
   is the order of the dependencies. */
static inline RunModes run_modes_resolve(const RunEnv &e, bool has_carr_in, bool has_carr_predict,
                                         bool carrier_int, int clamped_batch)
{
    auto is = [](const char *v, char c) { return v && v[0] == c; };
    auto eq = [](const char *v, const char *s) { return v && strcmp(v, s) == 0; };
    auto num = [](const char *v) { return v && *v ? atoi(v) : 0; };
    RunModes m;
    m.use_lin = !eq(e.path, "walk");
    m.force_exact = num(e.force_exact);
    m.late_verdicts = is(e.late_verdicts, '1');
    m.upload_dev = !eq(e.upload, "dma");
    m.rows_pool = !is(e.rows_pool, '0');
    m.spec_cus = num(e.spec_cus);
    m.render_rest = m.spec_cus > 0 && e.render_rest != nullptr;
    /* off: the configs[4] run measured 43.2-43.4 GB/s with them against 43.8-44.8 without
       (profiles/round5/e2e/probe_r5s) */
    m.dev_anch = is(e.dev_anchors, '1');
    /* spec <- use_lin, carrier: the chain is run ahead where the checkpoints are lazy, i.e. on the
       fast path with the float carrier (the integer-carrier chain records them for free) */
    m.spec = m.use_lin && !carrier_int && !is(e.spec, '0');
    /* rec <- spec, hand-off: a hand-off without a prediction callback has the exact carriers
       before its walks and takes the walks themselves (chain_upfront_spec) */
    m.rec = m.spec && !(has_carr_in && !has_carr_predict) && !is(e.rec, '0');
    /* anchors <- spec, hand-off: held wherever the per-batch chain could fill them */
    m.anchors = m.spec && m.use_lin && !has_carr_in && !is(e.anchors, '0');
    /* rows_ahead <- spec, hand-off, the clamped batch: the rows and prover threads where the
       planner is the limit, slots of >= 1024 blocks (-b 1 at 2.6 MS/s: 2,048).  The D2H-bound
       formats gain nothing from them, and inside bench.py's process the extra threads cost the
       -b 16 leg a third of its download rate (profiles/round3/e2e_planner/bench_*_r3af.log);
       GSS_RUN_ROWS_AHEAD=1 / 0 forces */
    const bool want_rows = e.rows_ahead && *e.rows_ahead ? e.rows_ahead[0] != '0'
                                                         : clamped_batch >= 1024;
    m.rows_ahead = m.spec && !has_carr_in && want_rows;
    /* proof_mode <- use_lin, rows_ahead, rec.  gpu: the proofs on the GPU, run ahead by the
       planner; host: on the host threads; split: every other slot on the GPU.  The default (auto)
       proves on the GPU only the planner-bound runs (rows ahead) with the walks' records (no
       walks on the host): there the host's CPUs are the limit and the proofs take them off it
       (configs[4] e2e 0.85-0.86 against 0.80-0.82 of the D2H ceiling,
       profiles/round5/e2e/b_*_r5q).  Elsewhere the two are even since the proof kernel spreads a
       small slot's channels over waves (configs[3]: 0.695-0.702 s against 0.695-0.705, the
       headline and configs[2] within noise; profiles/round5/e2e/r6e, e2e_modes_r6i.log), and
       host proofs keep the GPU's queues to the render and the copies */
    const int gpu_auto = m.rows_ahead && m.rec ? 1 : 0;
    m.proof_mode = !m.use_lin ? 0
                   : !e.proof || !*e.proof || eq(e.proof, "auto") ? gpu_auto
                   : eq(e.proof, "gpu") ? 1
                   : eq(e.proof, "split") ? 2 : 0;
    m.gpu_proof = m.proof_mode != 0;
    /* prover <- rows_ahead, use_lin, proof_mode: with every proof on the GPU it has no work */
    m.prover = m.rows_ahead && m.use_lin && m.proof_mode != 1 && !is(e.prover, '0');
    return m;
}

#endif
