/*
 * run_stages_check.cpp — the run's stage resolver (csrc/hip/gss_run_stages.h) with the host plane
 * alone: named cases for every refusal of run_stages_resolve (code and text, and which one comes
 * first when several apply) and for what it resolves (formats, block sizes, the second slot
 * buffer, the filter's lead blocks, the run's own copies of the options).  Test infrastructure
 * only (tests/test_run_stages.py builds and runs it).
 */
#include <stdio.h>
#include <string.h>
#include "gss_run_stages.h"

static int fails = 0;
static const StageLaunches ALL = {true, true, true, true};

static gss_scn_info_t scn(int fmt, int n_per_blk = 1000, int64_t next_block = 0)
{
    gss_scn_info_t i;
    memset(&i, 0, sizeof i);
    i.n_per_blk = n_per_blk;
    i.n_blocks = 3000;
    i.data_format = fmt;
    i.next_block = next_block;
    return i;
}

static const gss_impair_t NOISE = {1, 256 * 40, 2}, PLAIN = {0, 0, 0};

static gss_jam_t jam_ok()
{
    gss_jam_t j;
    memset(&j, 0, sizeof j);
    j.sweep = 1;
    j.amp = 65536;
    return j;
}

static gss_echo_t echo_ok()
{
    gss_echo_t e;
    memset(&e, 0, sizeof e);
    e.alpha_q16 = 32768;
    return e;
}

static gss_fir_t fir_ok(int n_taps)
{
    gss_fir_t f;
    memset(&f, 0, sizeof f);
    f.n_taps = n_taps;
    f.taps[n_taps / 2] = 16384;
    return f;
}

static int carr_in(void *, double *) { return 0; }

/* a refusal: its code, and its text from the first character on */
static void refused(const char *name, const gss_run_opts_t *o, const gss_scn_info_t &info,
                    int64_t first, int64_t n, const StageLaunches &have, int code, const char *text)
{
    RunStages g;
    const int rc = run_stages_resolve(o, info, first, n, have, &g);
    const char *got = rc ? gss_last_error() : "";
    const bool ok = rc == code && strncmp(got, text, strlen(text)) == 0;
    if (!ok)
        printf("  %s: rc %d \"%s\", expected %d \"%s\"\n", name, rc, got, code, text);
    printf("%-64s %s\n", name, ok ? "ok" : "FAIL");
    fails += !ok;
}

struct Want {
    int fmt, fmt_out;
    size_t bb, bb_r;
    bool needs_imp_buf;
    int64_t lead_blocks;
};

static void resolved(const char *name, const gss_run_opts_t *o, const gss_scn_info_t &info,
                     int64_t first, int64_t n, Want w)
{
    RunStages g;
    const int rc = run_stages_resolve(o, info, first, n, ALL, &g);
    bool ok = rc == 0;
    if (rc)
        printf("  %s: rc %d \"%s\"\n", name, rc, gss_last_error());
#define X(f)                                                                                 \
    if (!rc && (long long)g.f != (long long)w.f) {                                           \
        printf("  %s: %s = %lld, expected %lld\n", name, #f, (long long)g.f, (long long)w.f); \
        ok = false;                                                                          \
    }
    X(fmt) X(fmt_out) X(bb) X(bb_r) X(needs_imp_buf) X(lead_blocks)
#undef X
    if (!rc) {                                         /* what follows from the options given */
        const bool fir = o && o->fir;
        ok = ok && g.impair == (o ? o->impair : nullptr) && g.n_jam == (o ? o->n_jam : 0) &&
             g.n_echo == (o ? o->n_echo : 0) && g.has_fir == fir && stages_need_order(g) == fir;
    }
    printf("%-64s %s\n", name, ok ? "ok" : "FAIL");
    fails += !ok;
}

static void refusals()
{
    const gss_jam_t jam = jam_ok();
    const gss_echo_t echo = echo_ok();
    const gss_fir_t fir = fir_ok(33);
    const gss_scn_info_t s16 = scn(GSS_FMT_SC16);
    gss_run_opts_t o;
    auto clear = [&] { memset(&o, 0, sizeof o); };
    const char *t;

    t = "invalid format 3 for 1000 samples/block";
    refused("format: not a format", nullptr, scn(3), 0, -1, ALL, GSS_E_ARG, t);
    refused("format: SC01 blocks of 1002 samples", nullptr, scn(GSS_FMT_SC01, 1002), 0, -1, ALL,
            GSS_E_ARG, "invalid format 1 for 1002 samples/block");
    gss_impair_t bad = {1, 0x01000000u, 0};
    clear(); o.impair = &bad;
    refused("format before the impairment", &o, scn(3), 0, -1, ALL, GSS_E_ARG, t);

    t = "invalid impairment (sigma_q8 <= 0xFFFFFF, shift 0..8)";
    refused("impairment: sigma_q8 2^24", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    bad = {1, 256, -1};
    refused("impairment: shift -1", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    bad = {1, 256, 9};
    refused("impairment: shift 9", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    refused("impairment: invalid before no launch", &o, s16, 0, -1, {false, true, true, true},
            GSS_E_ARG, t);
    clear(); o.impair = &NOISE;
    refused("impairment: no launch", &o, s16, 0, -1, {false, true, true, true}, GSS_E_STATE,
            "additive noise requested, but this build has no impairment launch "
            "(gss_impair_device)");

    t = "invalid jammers (0..4 of them, with an impairment for the shift)";
    static_assert(GSS_MAXJAM == 4, "the texts below name the limit");
    clear(); o.impair = &NOISE; o.jam = &jam; o.n_jam = -1;
    refused("jammers: -1 of them", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.n_jam = GSS_MAXJAM + 1;
    refused("jammers: one too many", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.n_jam = 1; o.impair = nullptr;
    refused("jammers: no impairment", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.impair = &NOISE; o.jam = nullptr;
    refused("jammers: no array", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    gss_jam_t jbad = jam;
    jbad.sweep = 0;
    o.jam = &jbad;
    refused("jammers: sweep 0 (gss_jam_check)", &o, s16, 0, -1, ALL, GSS_E_ARG,
            "invalid jammer 0 (sweep >= 1, amp <= 2^23");
    refused("jammers: invalid before no launch", &o, s16, 0, -1, {true, false, true, true},
            GSS_E_ARG, "invalid jammer 0 (");
    o.jam = &jam;
    refused("jammers: no launch", &o, s16, 0, -1, {true, false, true, true}, GSS_E_STATE,
            "jammers requested, but this build has no jammer launch (gss_jam_device)");
    o.echo = &echo; o.n_echo = -1;
    refused("jammers: no launch before the echoes", &o, s16, 0, -1, {true, false, true, true},
            GSS_E_STATE, "jammers requested");

    t = "invalid echoes (0..4 of them, with an impairment for the shift)";
    static_assert(GSS_MAXECHO == 4, "the texts below name the limit");
    clear(); o.impair = &NOISE; o.echo = &echo; o.n_echo = -1;
    refused("echoes: -1 of them", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.n_echo = GSS_MAXECHO + 1;
    refused("echoes: one too many", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.n_echo = 1; o.impair = nullptr;
    refused("echoes: no impairment", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.impair = &NOISE; o.echo = nullptr;
    refused("echoes: no array", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    gss_echo_t ebad = echo;
    ebad.prn = 33;
    o.echo = &ebad;
    refused("echoes: prn 33 (gss_echo_check)", &o, s16, 0, -1, ALL, GSS_E_ARG,
            "invalid echo 0 (delay < 1023 * 2^32");
    o.echo = &echo;
    refused("echoes: no launch", &o, s16, 0, -1, {true, true, false, true}, GSS_E_STATE,
            "echoes requested, but this build has no echo launch (gss_echo_device)");
    o.fir = &fir; o.carr_in = carr_in;
    refused("echoes: no launch before the filter", &o, s16, 0, -1, {true, true, false, true},
            GSS_E_STATE, "echoes requested");

    t = "the filter needs an impairment (sigma_q8 = 0: none) and no carrier hand-off (carr_in)";
    clear(); o.fir = &fir;
    refused("filter: no impairment", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    o.impair = &PLAIN; o.carr_in = carr_in;
    refused("filter: with a carrier hand-off", &o, s16, 0, -1, ALL, GSS_E_ARG, t);
    gss_fir_t fbad = fir;
    fbad.n_taps = 0;
    clear(); o.impair = &PLAIN; o.fir = &fbad;
    refused("filter: 0 taps (gss_fir_check)", &o, s16, 0, -1, ALL, GSS_E_ARG,
            "invalid filter (1..");
    refused("filter: invalid before no launch", &o, s16, 0, -1, {true, true, true, false},
            GSS_E_ARG, "invalid filter (1..");
    o.fir = &fir;
    refused("filter: no launch", &o, s16, 0, -1, {true, true, true, false}, GSS_E_STATE,
            "a filter requested, but this build has no filter launch (gss_fir_device)");
    refused("filter: the scenario is past the lead block", &o, scn(GSS_FMT_SC16, 1000, 5), 5, 10,
            ALL, GSS_E_STATE,
            "a filtered run from block 5 needs block 4, but the scenario is at block 5");
    refused("filter: no launch before the lead block", &o, scn(GSS_FMT_SC16, 1000, 5), 5, 10,
            {true, true, true, false}, GSS_E_STATE, "a filter requested");
    const gss_fir_t wide = fir_ok(63);
    o.fir = &wide;
    refused("filter: short blocks, the scenario inside the lead", &o, scn(GSS_FMT_SC16, 8, 93), 100,
            -1, ALL, GSS_E_STATE,
            "a filtered run from block 100 needs block 92, but the scenario is at block 93");
}

static void resolutions()
{
    const gss_jam_t jam = jam_ok();
    const gss_echo_t echo = echo_ok();
    const gss_fir_t fir = fir_ok(33), wide = fir_ok(63), one = fir_ok(1);
    gss_run_opts_t o;
    memset(&o, 0, sizeof o);
    const int F16 = GSS_FMT_SC16, F08 = GSS_FMT_SC08, F01 = GSS_FMT_SC01;

    /* no stage: the blocks render at the scenario's format, one buffer */
    resolved("no options, SC16", nullptr, scn(F16), 0, -1, {F16, F16, 4000, 4000, false, 0});
    resolved("no options, SC08", nullptr, scn(F08), 7, 5, {F08, F08, 2000, 2000, false, 0});
    resolved("no options, SC01", nullptr, scn(F01), 0, -1, {F01, F01, 250, 250, false, 0});
    resolved("empty options, SC08", &o, scn(F08), 0, -1, {F08, F08, 2000, 2000, false, 0});
    o.carr_in = carr_in;
    resolved("a carrier hand-off alone, SC01", &o, scn(F01), 9, 9, {F01, F01, 250, 250, false, 0});

    /* noise: SC16 renders; in place at SC16, else a second buffer */
    memset(&o, 0, sizeof o);
    o.impair = &NOISE;
    resolved("noise, SC16 (in place)", &o, scn(F16), 0, -1, {F16, F16, 4000, 4000, false, 0});
    resolved("noise, SC08", &o, scn(F08), 0, -1, {F16, F08, 2000, 4000, true, 0});
    resolved("noise, SC01", &o, scn(F01), 0, -1, {F16, F01, 250, 4000, true, 0});
    resolved("noise, SC01, from block 50: no lead without a filter", &o, scn(F01), 50, 10,
             {F16, F01, 250, 4000, true, 0});
    o.carr_in = carr_in;
    resolved("noise with a carrier hand-off, SC08", &o, scn(F08), 50, 10,
             {F16, F08, 2000, 4000, true, 0});
    o.carr_in = nullptr;
    o.jam = &jam; o.n_jam = 1; o.echo = &echo; o.n_echo = 1;
    resolved("noise, a jammer and an echo, SC16", &o, scn(F16), 0, -1,
             {F16, F16, 4000, 4000, false, 0});
    resolved("noise, a jammer and an echo, SC08", &o, scn(F08), 0, -1,
             {F16, F08, 2000, 4000, true, 0});

    /* a filter: always the second buffer; the lead blocks hold the n_taps - 1 samples before */
    memset(&o, 0, sizeof o);
    o.impair = &PLAIN; o.fir = &fir;
    resolved("filter, SC16, from block 0", &o, scn(F16), 0, -1, {F16, F16, 4000, 4000, true, 0});
    resolved("filter, SC08, from block 0", &o, scn(F08), 0, 20, {F16, F08, 2000, 4000, true, 0});
    resolved("filter, SC01, from block 0", &o, scn(F01), 0, -1, {F16, F01, 250, 4000, true, 0});
    resolved("filter, SC16, from block 1", &o, scn(F16), 1, 10, {F16, F16, 4000, 4000, true, 1});
    resolved("filter, SC08, from block 1, to the end", &o, scn(F08), 1, -1,
             {F16, F08, 2000, 4000, true, 1});
    resolved("filter, SC01, from block 100", &o, scn(F01), 100, 10,
             {F16, F01, 250, 4000, true, 1});
    resolved("filter, from block 100, the scenario at block 99", &o, scn(F16, 1000, 99), 100, 10,
             {F16, F16, 4000, 4000, true, 1});
    resolved("filter, from block 100, an empty range: no lead", &o, scn(F16, 1000, 100), 100, 0,
             {F16, F16, 4000, 4000, true, 0});
    o.impair = &NOISE; o.jam = &jam; o.n_jam = 1;
    resolved("filter after noise and a jammer, SC08, from block 3", &o, scn(F08), 3, 4,
             {F16, F08, 2000, 4000, true, 1});
    o.jam = nullptr; o.n_jam = 0;
    o.fir = &one;
    resolved("filter of one tap, from block 100: no memory, no lead", &o, scn(F16, 1000, 100), 100,
             10, {F16, F16, 4000, 4000, true, 0});
    /* blocks shorter than the filter's memory: 62 samples before the range in blocks of 8 */
    o.fir = &wide;
    resolved("filter of 63 taps, blocks of 8, from block 100", &o, scn(F16, 8), 100, 10,
             {F16, F16, 32, 32, true, 8});
    resolved("filter of 63 taps, blocks of 8, from block 3: the run's start", &o, scn(F16, 8), 3,
             10, {F16, F16, 32, 32, true, 3});
    resolved("filter of 63 taps, blocks of 62, from block 100", &o, scn(F16, 62), 100, 10,
             {F16, F16, 248, 248, true, 1});
    resolved("filter of 63 taps, blocks of 61, from block 100", &o, scn(F16, 61), 100, 10,
             {F16, F16, 244, 244, true, 2});
}

/* the run keeps its own copies of the jammers, echoes and taps (the caller's may go) */
static void copies()
{
    gss_jam_t jam[2] = {jam_ok(), jam_ok()};
    gss_echo_t echo[2] = {echo_ok(), echo_ok()};
    gss_fir_t fir = fir_ok(33);
    jam[1].amp = 7;
    echo[1].prn = 5;
    gss_run_opts_t o;
    memset(&o, 0, sizeof o);
    o.impair = &NOISE;
    o.jam = jam; o.n_jam = 2; o.echo = echo; o.n_echo = 2; o.fir = &fir;
    RunStages g;
    bool ok = run_stages_resolve(&o, scn(GSS_FMT_SC08), 0, -1, ALL, &g) == 0;
    const gss_jam_t j1 = jam[1];
    const gss_echo_t e1 = echo[1];
    const gss_fir_t f = fir;
    memset(jam, 0xff, sizeof jam);
    memset(echo, 0xff, sizeof echo);
    memset(&fir, 0xff, sizeof fir);
    ok = ok && g.n_jam == 2 && memcmp(&g.jam[1], &j1, sizeof j1) == 0 && g.n_echo == 2 &&
         memcmp(&g.echo[1], &e1, sizeof e1) == 0 && g.has_fir && memcmp(&g.fir, &f, sizeof f) == 0 &&
         g.impair == &NOISE;
    printf("%-64s %s\n", "the run's copies of the jammers, echoes and taps", ok ? "ok" : "FAIL");
    fails += !ok;
}

int main()
{
    refusals();
    resolutions();
    copies();
    printf("%s\n", fails ? "FAILED" : "all cases ok");
    return fails ? 1 : 0;
}
