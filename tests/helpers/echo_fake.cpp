/*
 * echo_fake.cpp — gss_run with noise, a jammer and multipath echoes (gss_run_opts_t.impair, .jam,
 * .echo) on the CPU fakes of tests/helpers (fake_hip, fake_dev.cpp; see run_fake.cpp and
 * jam_fake.cpp).  The launches are stage_fake.h's: gss_echo_host, gss_jam_host and gss_impair_host
 * queued on the stream.  For each format the bytes of a run with noise, one jammer and two echoes
 * must be gss_jam_host over gss_echo_host over the bytes of the plain SC16 run of the same
 * scenario, with the rows and the nav table of a second scenario walked by gss_scn_next: so the
 * rows a slot uploads must carry their final carriers whatever the batch and the proof mode (the
 * redo of rejected blocks included), and a block range must be the matching slice.  A run with
 * n_echo = 0 makes no echo launch.  Built with -DNO_LAUNCH the echoes' launch is absent and the
 * run must refuse with GSS_E_STATE.  Test infrastructure only.
 *
 * usage: echo_fake NAV_FILE
 */
#ifdef NO_LAUNCH
#define STAGE_FAKE_NO_ECHO
#endif
#include "stage_fake.h"

static const char *g_nav;
static gss_scn *open_scn(double fs, int fmt) { return open_scn(g_nav, fs, fmt, 3.0); }

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: echo_fake NAV_FILE\n");
        return 2;
    }
    g_nav = argv[1];
    gss_dev *d = fake_dev_open();
    const gss_impair_t imp = {0x123456789abcdefull, 256 * 300, 1};
    gss_jam_t jam[1];
    gss_echo_t echo[2];
    /* a tone at 137 kHz, 10 dB, pulsed 3 of 10; an echo of every satellite 150 m late, 6 dB down,
       fading at 2.5 Hz; one of PRN 7 at 40 m, 3 dB down, in anti-phase */
    if (gss_jam_make(1.0e6, 10.0, 137.0e3, 0.0, 0.0, 10.0e-6, 0.3, &jam[0]) ||
        gss_echo_make(1.0e6, 0, 150.0, 6.0, 30.0, 2.5, &echo[0]) ||
        gss_echo_make(1.0e6, 7, 40.0, 3.0, 180.0, 0.0, &echo[1])) {
        printf("gss_jam_make / gss_echo_make: %s\n", gss_last_error());
        return 1;
    }
    gss_run_opts_t ro;
    memset(&ro, 0, sizeof ro);
    ro.impair = &imp;
    ro.jam = jam;
    ro.n_jam = 1;
    ro.echo = echo;
    ro.n_echo = 2;
#ifdef NO_LAUNCH
    {
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        const int rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &ro);
        gss_scn_close(s);
        printf("no launch: rc %d (%s)\n", rc, gss_last_error());
        if (rc != GSS_E_STATE || !k.bytes.empty() || g_impair_calls || g_jam_calls)
            return 1;
        printf("refused ok\n");
        return 0;
    }
#else
    /* echoes without an impairment, too many of them, an invalid one: refused before any launch */
    {
        gss_run_opts_t bad = ro;
        int rcs[3];
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        bad.impair = nullptr;
        bad.jam = nullptr;
        bad.n_jam = 0;
        rcs[0] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        bad = ro;
        bad.n_echo = GSS_MAXECHO + 1;
        rcs[1] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        gss_echo_t wrong[2] = {echo[0], echo[1]};
        wrong[1].delay = (uint64_t)1023 << 32;
        bad = ro;
        bad.echo = wrong;
        rcs[2] = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &bad);
        gss_scn_close(s);
        if (rcs[0] != GSS_E_ARG || rcs[1] != GSS_E_ARG || rcs[2] != GSS_E_ARG || !k.bytes.empty() ||
            g_echo_calls || g_jam_calls || g_impair_calls) {
            printf("argument errors: rc %d %d %d, %zu bytes FAIL\n", rcs[0], rcs[1], rcs[2],
                   k.bytes.size());
            return 1;
        }
        printf("argument errors ok\n");
    }
    std::vector<uint32_t> ca(32 * GSS_CA_WORDS);
    gss_ca_table(ca.data());
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
        rc = gss_echo_host(echo, 2, blk.data(), nch.data(), nblk, info.n_per_blk, ca.data(), 32, rows,
                           n_rows, 0, mid.data());
        gss_scn_close(s);
        std::vector<uint8_t> want(gss_fmt_bytes(n, c.fmt));
        if (rc || gss_jam_host(&imp, jam, 1, mid.data(), 0, n, c.fmt, want.data())) {
            printf("host echoes and jammer: %s\n", gss_last_error());
            return 1;
        }
        if (memcmp(mid.data(), plain.bytes.data(), 4 * n) == 0) {
            printf("the echoes changed nothing FAIL\n");
            return 1;
        }
        for (const Mode &m : modes) {
            stage_mode_env(&m);
            Sink k;
            g_impair_calls = g_echo_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, m.batch, 2, sink, &k, &ro);
            gss_scn_close(s);
            const bool ok = rc == 0 && k.bad == 0 && k.bytes == want && g_impair_calls == 0 &&
                            g_echo_calls > 0;
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
        /* no echo: no echo launch, and the jammer's bytes */
        {
            gss_run_opts_t none = ro;
            none.n_echo = 0;
            Sink k;
            g_echo_calls = g_jam_calls = 0;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &none);
            gss_scn_close(s);
            std::vector<uint8_t> w0(want.size());
            gss_jam_host(&imp, jam, 1, (const int16_t *)plain.bytes.data(), 0, n, c.fmt, w0.data());
            const bool ok = rc == 0 && k.bytes == w0 && g_echo_calls == 0 && g_jam_calls > 0;
            printf("-b %-2d no echo %s\n", c.fmt, ok ? "ok" : "FAIL");
            fails += !ok;
        }
    }
    fake_dev_close(d);
    if (fails)
        return 1;
    printf("all echoed runs ok\n");
    return 0;
#endif
}
