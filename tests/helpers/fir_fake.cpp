/*
 * fir_fake.cpp — gss_run with noise, a jammer, an echo and the front-end filter
 * (gss_run_opts_t.impair, .jam, .echo, .fir) on the CPU fakes of tests/helpers (fake_hip,
 * fake_dev.cpp; see run_fake.cpp and echo_fake.cpp).  The launches are stage_fake.h's: the host
 * statements queued on the stream.  For each format the bytes of such a run must be gss_fir_host
 * over gss_jam_host (to SC16) over gss_echo_host over the bytes of the plain SC16 run of the same
 * scenario, treated as one continuous stream with zeros before it: whatever the batch (a batch of
 * 1 puts every slot boundary on a block boundary), with device proofs and every third block on
 * the exact path, and with GSS_RUN_LATE_VERDICTS=1, which a filtered run overrides.  A block
 * range must be the matching slice.  fir = NULL makes no filter launch.  Built with -DNO_LAUNCH
 * the filter's launch is absent and the run must refuse with GSS_E_STATE.  Test infrastructure
 * only.
 *
 * usage: fir_fake NAV_FILE
 */
#ifdef NO_LAUNCH
#define STAGE_FAKE_NO_FIR
#endif
#include "stage_fake.h"

static const char *g_nav;
static gss_scn *open_scn(double fs, int fmt) { return open_scn(g_nav, fs, fmt, 1.2); }
static int no_carriers(void *, double *) { return 0; }

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: fir_fake NAV_FILE\n");
        return 2;
    }
    g_nav = argv[1];
    gss_dev *d = fake_dev_open();
    const gss_impair_t imp = {0x123456789abcdefull, 256 * 300, 1};
    gss_jam_t jam[1];
    gss_echo_t echo[1];
    gss_fir_t fir;
    /* a tone at 437 kHz, 10 dB; an echo of every satellite 150 m late, 6 dB down, fading at
       2.5 Hz; a 700 kHz filter of 63 taps */
    if (gss_jam_make(1.0e6, 10.0, 437.0e3, 0.0, 0.0, 0.0, 0.0, &jam[0]) ||
        gss_echo_make(1.0e6, 0, 150.0, 6.0, 30.0, 2.5, &echo[0]) ||
        gss_fir_make(1.0e6, 700.0e3, 63, &fir)) {
        printf("gss_jam_make / gss_echo_make / gss_fir_make: %s\n", gss_last_error());
        return 1;
    }
    gss_run_opts_t ro;
    memset(&ro, 0, sizeof ro);
    ro.impair = &imp;
    ro.jam = jam;
    ro.n_jam = 1;
    ro.echo = echo;
    ro.n_echo = 1;
    ro.fir = &fir;
#ifdef NO_LAUNCH
    {
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        const int rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &ro);
        gss_scn_close(s);
        printf("no launch: rc %d (%s)\n", rc, gss_last_error());
        if (rc != GSS_E_STATE || !k.bytes.empty() || g_impair_calls || g_jam_calls || g_echo_calls)
            return 1;
        printf("refused ok\n");
        return 0;
    }
#else
    /* a filter without an impairment, an invalid one (three ways), one with carr_in: refused
       before any launch */
    {
        int rcs[5];
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        gss_run_opts_t bad;
        memset(&bad, 0, sizeof bad);
        bad.fir = &fir;
        rcs[0] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        gss_fir_t wrong = fir;
        wrong.n_taps = 65;
        bad = ro;
        bad.fir = &wrong;
        rcs[1] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        wrong = fir;
        wrong.pad = 1;
        rcs[2] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        wrong = fir;
        wrong.taps[0] = 32767;
        wrong.taps[1] = -32767;
        rcs[3] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        bad = ro;
        bad.carr_in = no_carriers;
        rcs[4] = gss_run_ex(d, s, 2, 2, 8, 2, sink, &k, &bad);
        gss_scn_close(s);
        bool ok = k.bytes.empty() && !g_fir_calls && !g_echo_calls && !g_jam_calls && !g_impair_calls;
        for (int rc : rcs)
            ok = ok && rc == GSS_E_ARG;
        if (!ok) {
            printf("argument errors: rc %d %d %d %d %d, %zu bytes FAIL\n", rcs[0], rcs[1], rcs[2],
                   rcs[3], rcs[4], k.bytes.size());
            return 1;
        }
        printf("argument errors ok\n");
    }
    std::vector<uint32_t> ca(32 * GSS_CA_WORDS);
    gss_ca_table(ca.data());
    struct Case { double fs; int fmt; } cases[] = {{1000010.0, 16}, {1000010.0, 8}, {1.0e6, 1}};
    const Mode modes[] = {
        {"default", nullptr, nullptr, nullptr, 8},
        {"batch 1", nullptr, nullptr, nullptr, 1},
        {"batch 3", nullptr, nullptr, nullptr, 3},
        {"device proofs, every 3rd exact", "gpu", "3", "0", 5},
        {"device proofs, every 3rd exact, late", "gpu", "3", "1", 64},
        {"device proofs, every 3rd exact, late, batch 1", "gpu", "3", "1", 1},
    };
    int fails = 0;
    for (const Case &c : cases) {
        Sink plain;
        gss_scn *s = open_scn(c.fs, 16);
        gss_scn_info_t info;
        gss_scn_info(s, &info);
        int rc = gss_run(d, s, 0, -1, 7, 2, sink, &plain);
        gss_scn_close(s);
        if (rc || plain.bad) {
            printf("plain run: rc %d %s\n", rc, gss_last_error());
            return 1;
        }
        const size_t n = plain.bytes.size() / 4;
        const int nblk = (int)(n / (size_t)info.n_per_blk);
        /* the rows and the nav table: a second scenario, walked on the host */
        std::vector<gss_chan_blk_t> blk((size_t)nblk * GSS_MAXCH);
        std::vector<int32_t> nch((size_t)nblk);
        s = open_scn(c.fs, 16);
        int got = 0;
        for (int at = 0; at < nblk; at += got) {
            rc = gss_scn_next(s, nblk - at, blk.data() + (size_t)at * GSS_MAXCH, nch.data() + at,
                              nullptr, &got, 2);
            if (rc || got == 0) {
                printf("rows: rc %d after %d blocks %s\n", rc, at, gss_last_error());
                return 1;
            }
        }
        const uint32_t *rows = nullptr;
        int n_rows = 0;
        gss_scn_nav_table(s, &rows, &n_rows);
        std::vector<int16_t> mid((const int16_t *)plain.bytes.data(),
                                 (const int16_t *)plain.bytes.data() + 2 * n);
        rc = gss_echo_host(echo, 1, blk.data(), nch.data(), nblk, info.n_per_blk, ca.data(), 32, rows,
                           n_rows, 0, mid.data());
        gss_scn_close(s);
        std::vector<int16_t> jammed(2 * n);
        std::vector<uint8_t> want(gss_fmt_bytes(n, c.fmt));
        std::vector<uint8_t> unfiltered(want.size());
        if (rc || gss_jam_host(&imp, jam, 1, mid.data(), 0, n, 16, jammed.data()) ||
            gss_jam_host(&imp, jam, 1, mid.data(), 0, n, c.fmt, unfiltered.data()) ||
            gss_fir_host(&fir, jammed.data(), nullptr, n, c.fmt, want.data())) {
            printf("host echo, jammer and filter: %s\n", gss_last_error());
            return 1;
        }
        if (want == unfiltered) {
            printf("the filter changed nothing FAIL\n");
            return 1;
        }
        for (const Mode &m : modes) {
            stage_mode_env(&m);
            Sink k;
            g_impair_calls = g_fir_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, m.batch, 2, sink, &k, &ro);
            gss_scn_close(s);
            const bool ok = rc == 0 && k.bad == 0 && k.bytes == want && g_impair_calls == 0 &&
                            g_fir_calls > 0;
            printf("-b %-2d n_per_blk %d %-46s rc %d bytes %zu %s\n", c.fmt, info.n_per_blk, m.name,
                   rc, k.bytes.size(), ok ? "ok" : "FAIL");
            if (!ok) {
                if (rc)
                    printf("  error: %s\n", gss_last_error());
                fails++;
            }
        }
        stage_mode_env(nullptr);
        /* a block range of the run is the matching slice, whatever the batch */
        for (int batch : {3, 1, 8}) {
            Sink k;
            k.next = 3;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 3, 4, batch, 2, sink, &k, &ro);
            gss_scn_close(s);
            const size_t bb = gss_block_bytes(info.n_per_blk, c.fmt);
            const bool ok = rc == 0 && k.bad == 0 && k.bytes.size() == 4 * bb &&
                            memcmp(k.bytes.data(), want.data() + 3 * bb, 4 * bb) == 0;
            printf("-b %-2d blocks 3..6 batch %d %s\n", c.fmt, batch, ok ? "ok" : "FAIL");
            fails += !ok;
        }
        /* an empty range after block 0 renders no lead-in block: no launch, no bytes */
        {
            Sink k;
            g_fir_calls = g_jam_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 3, 0, 3, 2, sink, &k, &ro);
            gss_scn_close(s);
            const bool ok = rc == 0 && k.bytes.empty() && g_fir_calls == 0 && g_jam_calls == 0;
            printf("-b %-2d empty range %s\n", c.fmt, ok ? "ok" : "FAIL");
            fails += !ok;
        }
        /* a range the scenario has passed the block before: refused */
        {
            Sink k;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, 3, 3, 2, sink, &k, &ro);
            const int rc2 = gss_run_ex(d, s, 3, 2, 3, 2, sink, &k, &ro);
            gss_scn_close(s);
            const bool ok = rc == 0 && rc2 == GSS_E_STATE;
            printf("-b %-2d continued run refused %s\n", c.fmt, ok ? "ok" : "FAIL");
            fails += !ok;
        }
        /* no filter: no filter launch, and the jammer's bytes */
        {
            gss_run_opts_t none = ro;
            none.fir = nullptr;
            Sink k;
            g_fir_calls = g_jam_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &none);
            gss_scn_close(s);
            const bool ok = rc == 0 && k.bytes == unfiltered && g_fir_calls == 0 && g_jam_calls > 0;
            printf("-b %-2d no filter %s\n", c.fmt, ok ? "ok" : "FAIL");
            fails += !ok;
        }
    }
    fake_dev_close(d);
    if (fails)
        return 1;
    printf("all filtered runs ok\n");
    return 0;
#endif
}
