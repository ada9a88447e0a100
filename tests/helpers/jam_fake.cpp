/*
 * jam_fake.cpp — gss_run with noise and jammers (gss_run_opts_t.impair, .jam) on the CPU fakes of
 * tests/helpers (fake_hip, fake_dev.cpp; see run_fake.cpp and impair_fake.cpp).  The launches
 * are stage_fake.h's: gss_jam_host and gss_impair_host queued on the stream.  For each format the
 * bytes of a run with noise and two jammers must be gss_jam_host over the bytes of the plain SC16
 * run of the same scenario, whatever the batch and the proof mode (the redo of rejected blocks
 * included), and a run with an impairment and no jammer must still take the impairment's launch.
 * Built with -DNO_LAUNCH the jammers' launch is absent and the run must refuse with GSS_E_STATE.
 * Test infrastructure only.
 *
 * usage: jam_fake NAV_FILE
 */
#ifdef NO_LAUNCH
#define STAGE_FAKE_NO_JAM
#endif
#include "stage_fake.h"

static const char *g_nav;
static gss_scn *open_scn(double fs, int fmt) { return open_scn(g_nav, fs, fmt, 3.0); }

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: jam_fake NAV_FILE\n");
        return 2;
    }
    g_nav = argv[1];
    gss_dev *d = fake_dev_open();
    const gss_impair_t imp = {0x123456789abcdefull, 256 * 300, 1};
    gss_jam_t jam[2];
    /* a tone at 137 kHz, 10 dB, pulsed 3 of 10; a sweep -400..+400 kHz in 137 samples, 0 dB */
    if (gss_jam_make(1.0e6, 10.0, 137.0e3, 0.0, 0.0, 10.0e-6, 0.3, &jam[0]) ||
        gss_jam_make(1.0e6, 0.0, -400.0e3, 400.0e3, 137.0e-6, 0.0, 0.0, &jam[1])) {
        printf("gss_jam_make: %s\n", gss_last_error());
        return 1;
    }
    jam[0].gate_shift = 7;
    jam[1].phase0 = 0x8000000000000001ull;
    gss_run_opts_t ro;
    memset(&ro, 0, sizeof ro);
    ro.impair = &imp;
    ro.jam = jam;
    ro.n_jam = 2;
#ifdef NO_LAUNCH
    {
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        const int rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &ro);
        gss_scn_close(s);
        printf("no launch: rc %d (%s)\n", rc, gss_last_error());
        if (rc != GSS_E_STATE || !k.bytes.empty() || g_impair_calls)
            return 1;
        printf("refused ok\n");
        return 0;
    }
#else
    /* jammers without an impairment, too many of them, an invalid one: refused before any launch */
    {
        gss_run_opts_t bad = ro;
        int rcs[3];
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        bad.impair = nullptr;
        rcs[0] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        bad = ro;
        bad.n_jam = GSS_MAXJAM + 1;
        rcs[1] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        gss_jam_t wrong[2] = {jam[0], jam[1]};
        wrong[1].sweep = 0;
        bad = ro;
        bad.jam = wrong;
        rcs[2] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        gss_scn_close(s);
        if (rcs[0] != GSS_E_ARG || rcs[1] != GSS_E_ARG || rcs[2] != GSS_E_ARG || !k.bytes.empty() ||
            g_jam_calls || g_impair_calls) {
            printf("argument errors: rc %d %d %d, %zu bytes FAIL\n", rcs[0], rcs[1], rcs[2],
                   k.bytes.size());
            return 1;
        }
        printf("argument errors ok\n");
    }
    struct Case { double fs; int fmt; } cases[] = {{1000010.0, 16}, {1000010.0, 8}, {1.0e6, 1}};
    const Mode modes[] = {
        {"default", nullptr, nullptr, nullptr, 8},
        {"device proofs, every 3rd exact", "gpu", "3", "0", 5},
        {"device proofs, every 3rd exact, redo", "gpu", "3", "1", 64},
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
        std::vector<uint8_t> want(gss_fmt_bytes(n, c.fmt));
        if (gss_jam_host(&imp, jam, 2, (const int16_t *)plain.bytes.data(), 0, n, c.fmt,
                         want.data())) {
            printf("host jammers: %s\n", gss_last_error());
            return 1;
        }
        for (const Mode &m : modes) {
            stage_mode_env(&m);
            Sink k;
            g_impair_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, m.batch, 2, sink, &k, &ro);
            gss_scn_close(s);
            const bool ok = rc == 0 && k.bad == 0 && k.bytes == want && g_impair_calls == 0;
            printf("-b %-2d n_per_blk %d %-40s rc %d bytes %zu %s\n", c.fmt, info.n_per_blk, m.name,
                   rc, k.bytes.size(), ok ? "ok" : "FAIL");
            if (!ok) {
                if (rc)
                    printf("  error: %s\n", gss_last_error());
                fails++;
            }
        }
        stage_mode_env(nullptr);
        /* a block range of the run is the matching slice */
        {
            Sink k;
            k.next = 3;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 3, 4, 3, 2, sink, &k, &ro);
            gss_scn_close(s);
            const size_t bb = gss_block_bytes(info.n_per_blk, c.fmt);
            const bool ok = rc == 0 && k.bad == 0 && k.bytes.size() == 4 * bb &&
                            memcmp(k.bytes.data(), want.data() + 3 * bb, 4 * bb) == 0;
            printf("-b %-2d blocks 3..6 %s\n", c.fmt, ok ? "ok" : "FAIL");
            fails += !ok;
        }
        /* no jammer: the impairment's own launch, and its bytes */
        {
            gss_run_opts_t none = ro;
            none.jam = nullptr;
            none.n_jam = 0;
            Sink k;
            g_impair_calls = g_jam_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &none);
            gss_scn_close(s);
            std::vector<uint8_t> w0(want.size());
            gss_impair_host(&imp, (const int16_t *)plain.bytes.data(), 0, n, c.fmt, w0.data());
            const bool ok = rc == 0 && k.bytes == w0 && g_jam_calls == 0 && g_impair_calls > 0;
            printf("-b %-2d no jammer %s\n", c.fmt, ok ? "ok" : "FAIL");
            fails += !ok;
        }
    }
    fake_dev_close(d);
    if (fails)
        return 1;
    printf("all jammed runs ok\n");
    return 0;
#endif
}
