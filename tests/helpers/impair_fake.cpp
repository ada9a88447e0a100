/*
 * impair_fake.cpp — gss_run with additive noise (gss_run_opts_t.impair) on the CPU fakes of
 * tests/helpers (fake_hip, fake_dev.cpp; see run_fake.cpp).  The impairment's launch is stage_fake.h's:
 * gss_impair_host queued on the stream.  For each format the bytes of an impaired run must
 * be gss_impair_host over the bytes of the plain SC16 run of the same scenario, whatever the
 * batch and the proof mode (the redo of rejected blocks included).  Built with -DNO_LAUNCH the
 * launch is absent and the run must refuse with GSS_E_STATE.  Test infrastructure only.
 *
 * usage: impair_fake NAV_FILE
 */
#ifdef NO_LAUNCH
#define STAGE_FAKE_NO_IMPAIR
#endif
#include "stage_fake.h"

static const char *g_nav;
static gss_scn *open_scn(double fs, int fmt) { return open_scn(g_nav, fs, fmt, 3.0); }

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: impair_fake NAV_FILE\n");
        return 2;
    }
    g_nav = argv[1];
    gss_dev *d = fake_dev_open();
    const gss_impair_t imp = {0x123456789abcdefull, 256 * 300, 1};
    gss_run_opts_t ro;
    memset(&ro, 0, sizeof ro);
    ro.impair = &imp;
#ifdef NO_LAUNCH
    {
        gss_scn *s = open_scn(1.0e6, 8);
        Sink k;
        const int rc = gss_run_ex(d, s, 0, -1, 8, 2, sink, &k, &ro);
        gss_scn_close(s);
        printf("no launch: rc %d (%s)\n", rc, gss_last_error());
        if (rc != GSS_E_STATE || !k.bytes.empty())
            return 1;
        printf("refused ok\n");
        return 0;
    }
#else
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
        if (gss_impair_host(&imp, (const int16_t *)plain.bytes.data(), 0, n, c.fmt, want.data())) {
            printf("host impairment: %s\n", gss_last_error());
            return 1;
        }
        for (const Mode &m : modes) {
            stage_mode_env(&m);
            Sink k;
            s = open_scn(c.fs, c.fmt);
            rc = gss_run_ex(d, s, 0, -1, m.batch, 2, sink, &k, &ro);
            gss_scn_close(s);
            const bool ok = rc == 0 && k.bad == 0 && k.bytes == want;
            printf("-b %-2d n_per_blk %d %-40s rc %d bytes %zu %s\n", c.fmt, info.n_per_blk, m.name,
                   rc, k.bytes.size(), ok ? "ok" : "FAIL");
            if (!ok) {
                if (rc)
                    printf("  error: %s\n", gss_last_error());
                fails++;
            }
        }
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
    }
    fake_dev_close(d);
    if (fails)
        return 1;
    printf("all impaired runs ok\n");
    return 0;
#endif
}
