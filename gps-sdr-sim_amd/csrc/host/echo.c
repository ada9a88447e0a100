/*
 * echo.c — the multipath echoes on the host: the plain-C statement of csrc/common/gss_echo.h over
 * the SC16 render of a run of blocks (gss_echo_host), the argument check it shares with the
 * launch (gss_echo_check), and gss_echo_make, which turns physical parameters into a gss_echo_t
 * once for the CLI and the binding.  The reference has no multipath model; like the noise and the
 * jammers this is an extension applied to its 16-bit samples before the quantise/pack epilogue
 * (gpssim.c:2266-2288), made from the channel rows its sample loop reads (gpssim.c:2190-2256).
 * gss_echo_host is what the GPU kernels (csrc/hip/gss_echo.hip) are tested against.
 */
#include <math.h>
#include <pthread.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_echo.h"

static uint32_t echo_lut[GSS_JAM_LUT];
static pthread_once_t echo_once = PTHREAD_ONCE_INIT;

static void echo_tables_make(void)
{
    int32_t s[512], c[512];
    gss_lut(s, c);
    for (int i = 0; i < GSS_JAM_LUT; i++)
        echo_lut[i] = gss_jam_cell(c[i], s[i]);
}

int gss_echo_check(const gss_echo_t *echo, int n_echo)
{
    if (n_echo < 0 || n_echo > GSS_MAXECHO || (n_echo > 0 && !echo))
        return gss_fail(GSS_E_ARG, "invalid echoes (0..%d of them)", GSS_MAXECHO);
    for (int i = 0; i < n_echo; i++) {
        const gss_echo_t *e = &echo[i];
        if (e->delay >= GSS_ECHO_DELAY_END || e->alpha_q16 > GSS_ECHO_ALPHA_MAX || e->prn < 0 ||
            e->prn > 32)
            return gss_fail(GSS_E_ARG, "invalid echo %d (delay < 1023 * 2^32, alpha_q16 <= 2^18, "
                                       "prn 0..32)", i);
    }
    return 0;
}

/* the checks of gss_echo_host and gss_echo_device on what the host can see */
int gss_echo_args(const gss_echo_t *echo, int n_echo, const void *blk, const void *nch, int nblk,
                  int n_per_blk, const void *ca_bits, int n_ca, const void *nav, int n_nav,
                  uint64_t sample0, const void *iq)
{
    const int rc = gss_echo_check(echo, n_echo);
    if (rc)
        return rc;
    if (nblk < 0 || n_per_blk < 1 || n_ca < 1 || n_nav < 1 ||
        (nblk > 0 && (!blk || !nch || !ca_bits || !nav || !iq)))
        return gss_fail(GSS_E_ARG, "invalid echo arguments");
    const uint64_t n = (uint64_t)nblk * (uint64_t)n_per_blk;
    if (sample0 + n < sample0)
        return gss_fail(GSS_E_ARG, "echo sample range passes 2^64");
    return 0;
}

int gss_echo_host(const gss_echo_t *echo, int n_echo, const gss_chan_blk_t *blk,
                  const int32_t *nch, int nblk, int n_per_blk, const uint32_t *ca_bits, int n_ca,
                  const uint32_t *nav, int n_nav, uint64_t sample0, int16_t *iq)
{
    int rc = gss_echo_args(echo, n_echo, blk, nch, nblk, n_per_blk, ca_bits, n_ca, nav, n_nav,
                           sample0, iq);
    if (rc)
        return rc;
    for (int b = 0; b < nblk; b++)
        if (nch[b] < 0 || nch[b] > GSS_MAXCH)
            return gss_fail(GSS_E_ARG, "invalid channel count %d in block %d", nch[b], b);
    pthread_once(&echo_once, echo_tables_make);
    for (int b = 0; b < nblk; b++) {
        gss_echo_row_t row[GSS_MAXECHO * GSS_MAXCH];
        gss_echo_state_t st[GSS_MAXECHO * GSS_MAXCH];
        const uint64_t base = sample0 + (uint64_t)b * (uint64_t)n_per_blk;
        int np = 0;
        for (int j = 0; j < n_echo; j++)
            for (int k = 0; k < nch[b]; k++)
                np += gss_echo_row(&echo[j], &blk[(size_t)b * GSS_MAXCH + k], base, n_ca, n_nav,
                                   &row[np]);
        for (int p = 0; p < np; p++)
            gss_echo_seed(&row[p], nav + (size_t)row[p].nav_tbl * GSS_NAV_WORDS, 0, &st[p]);
        int16_t *x = iq + 2 * (size_t)b * (size_t)n_per_blk;
        for (int s = 0; s < n_per_blk && np > 0; s++) {
            int32_t e[2] = {0, 0};
            for (int p = 0; p < np; p++) {
                gss_echo_add(&st[p], ca_bits + (size_t)row[p].ca_tbl * GSS_CA_WORDS, echo_lut,
                             &e[0], &e[1]);
                if (s + 1 < n_per_blk)
                    gss_echo_next(&row[p], nav + (size_t)row[p].nav_tbl * GSS_NAV_WORDS, &st[p]);
            }
            x[2 * s] = (int16_t)gss_echo_mix(x[2 * s], e[0]);
            x[2 * s + 1] = (int16_t)gss_echo_mix(x[2 * s + 1], e[1]);
        }
    }
    return 0;
}

int gss_echo_make(double fs_hz, int prn, double delay_m, double atten_db, double phase_deg,
                  double doppler_hz, gss_echo_t *out)
{
    if (!out || !isfinite(fs_hz) || !(fs_hz > 0.0) || prn < 0 || prn > 32 || !isfinite(delay_m) ||
        !isfinite(atten_db) || !isfinite(phase_deg) || !isfinite(doppler_hz))
        return gss_fail(GSS_E_ARG, "invalid echo parameters");
    gss_echo_t e;
    memset(&e, 0, sizeof e);
    const double delay = floor(delay_m * 1023000.0 / 299792458.0 * 4294967296.0 + 0.5);
    if (!(delay >= 0.0 && delay < 1023.0 * 4294967296.0))
        return gss_fail(GSS_E_ARG, "echo delay outside 0..1023 chips (0..299.8 km)");
    const double alpha = floor(65536.0 * pow(10.0, -atten_db / 20.0) + 0.5);
    if (!(alpha <= (double)GSS_ECHO_ALPHA_MAX))
        return gss_fail(GSS_E_ARG, "echo level out of range (at most 12.04 dB above the signal)");
    if (!(fabs(doppler_hz) < fs_hz / 2.0))
        return gss_fail(GSS_E_ARG, "echo Doppler outside (-fs/2, fs/2)");
    const double t = phase_deg / 360.0;
    const double th = (t - floor(t)) * 18446744073709551616.0;
    e.delay = (uint64_t)delay;
    e.alpha_q16 = (uint32_t)alpha;
    e.theta0 = th >= 18446744073709551616.0 ? 0u : (uint64_t)th;
    e.dstep = (uint64_t)(int64_t)floor(doppler_hz / fs_hz * 18446744073709551616.0 + 0.5);
    e.prn = prn;
    *out = e;
    return 0;
}
