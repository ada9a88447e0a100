/*
 * stage_fake.h — what impair_fake.cpp, jam_fake.cpp, echo_fake.cpp and fir_fake.cpp share: the
 * launches of the post-render stages on the CPU fakes of tests/helpers (fake_hip, fake_dev.cpp;
 * see run_fake.cpp), each the stage's host statement queued on the stream with a count of its
 * calls, and the scenario, sink and run-mode switches those programs drive gss_run with.  A
 * program leaves a launch out with STAGE_FAKE_NO_IMPAIR, _NO_JAM, _NO_ECHO or _NO_FIR defined
 * before this file (its -DNO_LAUNCH build: gss_run must then refuse).  Test infrastructure only.
 */
#ifndef STAGE_FAKE_H
#define STAGE_FAKE_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "gpssim_amd.h"
#include "fake_dev.h"
#include "../../gps-sdr-sim_amd/csrc/common/gss_stage.h"      /* gss_fmt_bytes */

static int g_impair_calls, g_jam_calls, g_echo_calls, g_fir_calls;

#ifndef STAGE_FAKE_NO_IMPAIR
extern "C" int gss_impair_device(gss_dev *d, const gss_impair_t *p, const int16_t *iq,
                                 uint64_t sample0, size_t n, int fmt, void *out, void *stream)
{
    if (!d || !p || !iq || !out)
        return GSS_E_ARG;
    g_impair_calls++;
    const gss_impair_t imp = *p;
    fake_enqueue((hipStream_t)stream, [=] {
        if (gss_impair_host(&imp, iq, sample0, n, fmt, out))
            abort();
    });
    return 0;
}
#endif

#ifndef STAGE_FAKE_NO_JAM
extern "C" int gss_jam_device(gss_dev *d, const gss_impair_t *p, const gss_jam_t *jam, int n_jam,
                              const int16_t *iq, uint64_t sample0, size_t n, int fmt, void *out,
                              void *stream)
{
    if (!d || !p || !jam || n_jam < 1 || n_jam > GSS_MAXJAM || !iq || !out)
        return GSS_E_ARG;
    g_jam_calls++;
    const gss_impair_t imp = *p;
    std::vector<gss_jam_t> js(jam, jam + n_jam);       /* read before the call returns */
    fake_enqueue((hipStream_t)stream, [=] {
        if (gss_jam_host(&imp, js.data(), (int)js.size(), iq, sample0, n, fmt, out))
            abort();
    });
    return 0;
}
#endif

#ifndef STAGE_FAKE_NO_ECHO
extern "C" int gss_echo_device(gss_dev *d, const gss_echo_t *echo, int n_echo,
                               const gss_chan_blk_t *blk, const int32_t *nch, int nblk,
                               int n_per_blk, const uint32_t *ca_bits, int n_ca,
                               const uint32_t *nav, int n_nav, uint64_t sample0, int16_t *iq,
                               void *stream)
{
    if (!d || !echo || n_echo < 1 || n_echo > GSS_MAXECHO || !blk || !nch || !ca_bits || !nav || !iq)
        return GSS_E_ARG;
    g_echo_calls++;
    std::vector<gss_echo_t> es(echo, echo + n_echo);   /* read before the call returns */
    fake_enqueue((hipStream_t)stream, [=] {            /* the rows are read when the stream runs */
        if (gss_echo_host(es.data(), (int)es.size(), blk, nch, nblk, n_per_blk, ca_bits, n_ca, nav,
                          n_nav, sample0, iq))
            abort();
    });
    return 0;
}
#endif

#ifndef STAGE_FAKE_NO_FIR
extern "C" int gss_fir_device(gss_dev *d, const gss_fir_t *fir, const int16_t *in,
                              const int16_t *halo, size_t n, int fmt, void *out, void *stream)
{
    if (!d || !fir || !in || !out)
        return GSS_E_ARG;
    g_fir_calls++;
    const gss_fir_t f = *fir;                          /* read before the call returns */
    fake_enqueue((hipStream_t)stream, [=] {            /* the halo is read when the stream runs */
        if (gss_fir_host(&f, in, halo, n, fmt, out))
            abort();
    });
    return 0;
}
#endif

static gss_scn *open_scn(const char *nav, double fs, int fmt, double duration)
{
    gss_opts_t o;
    memset(&o, 0, sizeof o);
    o.nav_file = nav;
    o.has_llh = 1;
    o.llh[0] = 30.286502;
    o.llh[1] = 120.032669;
    o.llh[2] = 100.0;
    o.samp_freq = fs;
    o.data_format = fmt;
    o.duration = duration;
    o.quiet = 1;
    gss_scn *s = nullptr;
    if (gss_scn_open(&s, &o)) {
        fprintf(stderr, "scenario: %s\n", gss_last_error());
        exit(2);
    }
    return s;
}

struct Sink {
    std::vector<uint8_t> bytes;
    int64_t next = 0;
    int bad = 0;
};

static int sink(void *user, const void *bytes, size_t n, int64_t first, int nb)
{
    Sink *k = (Sink *)user;
    if (first != k->next)
        k->bad++;
    k->next = first + nb;
    k->bytes.insert(k->bytes.end(), (const uint8_t *)bytes, (const uint8_t *)bytes + n);
    return 0;
}

/* a run mode: GSS_RUN_PROOF, GSS_RUN_FORCE_EXACT and GSS_RUN_LATE_VERDICTS (null: unset) and the
   batch.  stage_mode_env(nullptr) unsets the three */
struct Mode {
    const char *name, *proof, *exact, *late;
    int batch;
};

static void stage_mode_env(const Mode *m)
{
    const char *keys[] = {"GSS_RUN_PROOF", "GSS_RUN_FORCE_EXACT", "GSS_RUN_LATE_VERDICTS"};
    const char *vals[] = {m ? m->proof : nullptr, m ? m->exact : nullptr, m ? m->late : nullptr};
    for (int i = 0; i < 3; i++) {
        if (vals[i])
            setenv(keys[i], vals[i], 1);
        else
            unsetenv(keys[i]);
    }
}

#endif /* STAGE_FAKE_H */
