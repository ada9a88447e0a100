/*
 * run_modes_check.cpp — the run's mode resolver (csrc/hip/gss_run_modes.h) alone: named cases
 * against the modes the documentation gives for them (gss_run.hip's switch table, DESIGN.md §5.0,
 * §7.1, §7.2), and the invariants the rest of gss_run.hip relies on over the whole product of
 * switch values.  Test infrastructure only (tests/test_run_modes.py builds and runs it).
 */
#include <stdio.h>
#include <vector>
#include "gss_run_modes.h"

static int fails = 0;

struct Case {
    const char *name;
    RunEnv env;
    bool carr_in, carr_predict, carrier_int;
    int batch;
    RunModes want;
};

/* the modes of a default run of a float-carrier scenario at 100-block slots: the fast path, the
   chain run ahead with records, anchors held, rows on the planner, host proofs on the planner */
static RunModes base()
{
    RunModes m;
    m.use_lin = 1;
    m.force_exact = 0;
    m.late_verdicts = 0;
    m.upload_dev = 1;
    m.spec = 1;
    m.rec = 1;
    m.dev_anch = 0;
    m.anchors = 1;
    m.rows_ahead = 0;
    m.rows_pool = 1;
    m.proof_mode = 0;
    m.gpu_proof = 0;
    m.prover = 0;
    m.spec_cus = 0;
    m.render_rest = 0;
    return m;
}

#define FIELDS(X)                                                                            \
    X(use_lin) X(force_exact) X(late_verdicts) X(upload_dev) X(spec) X(rec) X(dev_anch)      \
    X(anchors) X(rows_ahead) X(rows_pool) X(proof_mode) X(gpu_proof) X(prover) X(spec_cus)   \
    X(render_rest)

static void check_case(const Case &c)
{
    const RunModes got =
        run_modes_resolve(c.env, c.carr_in, c.carr_predict, c.carrier_int, c.batch);
    bool ok = true;
#define X(f)                                                                                 \
    if (got.f != c.want.f) {                                                                 \
        printf("  %s: %s = %d, expected %d\n", c.name, #f, got.f, c.want.f);                 \
        ok = false;                                                                          \
    }
    FIELDS(X)
#undef X
    printf("%-60s %s\n", c.name, ok ? "ok" : "FAIL");
    fails += !ok;
}

static std::vector<Case> cases()
{
    std::vector<Case> v;
    auto add = [&](const char *name, RunEnv env, bool in, bool predict, bool cint, int batch,
                   RunModes want) { v.push_back({name, env, in, predict, cint, batch, want}); };
    RunEnv e;
    RunModes w;

    add("defaults, float carrier, batch 100", RunEnv(), false, false, false, 100, base());

    w = base();                       /* slots of >= 1024 blocks: rows thread, GPU proofs */
    w.rows_ahead = 1, w.proof_mode = 1, w.gpu_proof = 1;
    add("defaults, batch 2048", RunEnv(), false, false, false, 2048, w);

    e = RunEnv(), e.proof = "host";
    w = base(), w.rows_ahead = 1, w.prover = 1;
    add("batch 2048, GSS_RUN_PROOF=host: prover thread", e, false, false, false, 2048, w);
    e.prover = "0", w.prover = 0;
    add("batch 2048, GSS_RUN_PROOF=host, GSS_RUN_PROVER=0", e, false, false, false, 2048, w);

    e = RunEnv(), e.path = "walk";
    w = base(), w.use_lin = 0, w.spec = 0, w.rec = 0, w.anchors = 0;
    add("GSS_PATH=walk, batch 100", e, false, false, false, 100, w);
    add("GSS_PATH=walk, batch 2048", e, false, false, false, 2048, w);
    e.proof = "gpu";
    add("GSS_PATH=walk, GSS_RUN_PROOF=gpu: still no proofs", e, false, false, false, 2048, w);

    w = base(), w.spec = 0, w.rec = 0, w.anchors = 0;
    add("integer carrier, batch 100", RunEnv(), false, false, true, 100, w);
    add("integer carrier, batch 2048", RunEnv(), false, false, true, 2048, w);

    w = base(), w.rec = 0, w.anchors = 0;
    add("carr_in without carr_predict", RunEnv(), true, false, false, 100, w);
    add("carr_in without carr_predict, batch 2048", RunEnv(), true, false, false, 2048, w);
    w.rec = 1;
    add("carr_in with carr_predict", RunEnv(), true, true, false, 100, w);
    add("carr_in with carr_predict, batch 2048", RunEnv(), true, true, false, 2048, w);

    e = RunEnv(), e.spec = "0";
    w = base(), w.spec = 0, w.rec = 0, w.anchors = 0;
    add("GSS_RUN_SPEC=0", e, false, false, false, 100, w);
    add("GSS_RUN_SPEC=0, batch 2048", e, false, false, false, 2048, w);

    e = RunEnv(), e.rec = "0";
    w = base(), w.rec = 0;
    add("GSS_RUN_REC=0: anchors on", e, false, false, false, 100, w);
    e.anchors = "0", w.anchors = 0;
    add("GSS_RUN_REC=0, GSS_RUN_ANCHORS=0", e, false, false, false, 100, w);

    e = RunEnv(), e.rec = "0";        /* rows ahead without records: auto keeps host proofs */
    w = base(), w.rec = 0, w.rows_ahead = 1, w.prover = 1;
    add("GSS_RUN_REC=0, batch 2048", e, false, false, false, 2048, w);

    e = RunEnv(), e.proof = "split";
    w = base(), w.proof_mode = 2, w.gpu_proof = 1;
    add("GSS_RUN_PROOF=split, batch 100", e, false, false, false, 100, w);
    w.rows_ahead = 1, w.prover = 1;   /* the host's half of the slots on the prover thread */
    add("GSS_RUN_PROOF=split, batch 2048", e, false, false, false, 2048, w);

    e = RunEnv(), e.proof = "gpu";
    w = base(), w.proof_mode = 1, w.gpu_proof = 1;
    add("GSS_RUN_PROOF=gpu, batch 100", e, false, false, false, 100, w);

    e = RunEnv(), e.rows_ahead = "0";
    add("GSS_RUN_ROWS_AHEAD=0, batch 2048: auto gives host proofs", e, false, false, false, 2048,
        base());
    e = RunEnv(), e.rows_ahead = "1";
    w = base(), w.rows_ahead = 1, w.proof_mode = 1, w.gpu_proof = 1;
    add("GSS_RUN_ROWS_AHEAD=1, batch 100", e, false, false, false, 100, w);

    e = RunEnv(), e.force_exact = "7", e.late_verdicts = "1", e.upload = "dma";
    e.rows_pool = "0", e.dev_anchors = "1", e.spec_cus = "32", e.render_rest = "1";
    w = base(), w.force_exact = 7, w.late_verdicts = 1, w.upload_dev = 0, w.rows_pool = 0;
    w.dev_anch = 1, w.spec_cus = 32, w.render_rest = 1;
    add("the switches that stand alone", e, false, false, false, 100, w);
    e = RunEnv(), e.render_rest = "1";
    add("GSS_RUN_RENDER_REST without GSS_RUN_SPEC_CUS", e, false, false, false, 100, base());
    return v;
}

/* what gss_run.hip relies on, whatever the switches say */
static void check_invariants()
{
    const char *const spec_v[] = {nullptr, "0", "1"}, *const rec_v[] = {nullptr, "0", "1"};
    const char *const anch_v[] = {nullptr, "0"}, *const ra_v[] = {nullptr, "", "0", "1"};
    const char *const proof_v[] = {nullptr, "", "auto", "host", "gpu", "split", "other"};
    const char *const prover_v[] = {nullptr, "0", "1"}, *const path_v[] = {nullptr, "walk", "fast"};
    const char *const da_v[] = {nullptr, "1"};
    long n = 0, bad = 0;
    RunEnv e;
    for (const char *sp : spec_v) for (const char *re : rec_v) for (const char *an : anch_v)
    for (const char *ra : ra_v) for (const char *pf : proof_v) for (const char *pv : prover_v)
    for (const char *pa : path_v) for (const char *da : da_v)
    for (int hand = 0; hand < 3; hand++) for (int cint = 0; cint < 2; cint++)
    for (int batch : {100, 2048}) {
        e.spec = sp, e.rec = re, e.anchors = an, e.rows_ahead = ra, e.proof = pf, e.prover = pv;
        e.path = pa, e.dev_anchors = da;
        const bool in = hand > 0;
        const RunModes m = run_modes_resolve(e, in, hand == 2, cint != 0, batch);
        const bool ok = (!m.rec || m.spec) && (!m.spec || (m.use_lin && !cint)) &&
                        (!m.rows_ahead || (m.spec && !in)) &&
                        (!m.prover || (m.rows_ahead && m.use_lin && m.proof_mode != 1)) &&
                        ((m.gpu_proof != 0) == (m.proof_mode != 0)) &&
                        (!m.gpu_proof || m.use_lin) && (!m.anchors || (m.spec && !in));
        n++;
        bad += !ok;
    }
    printf("%-60s %s (%ld combinations, %ld bad)\n", "invariants", bad ? "FAIL" : "ok", n, bad);
    fails += bad != 0;
}

int main()
{
    for (const Case &c : cases())
        check_case(c);
    check_invariants();
    printf("%s\n", fails ? "FAILED" : "all cases ok");
    return fails ? 1 : 0;
}
