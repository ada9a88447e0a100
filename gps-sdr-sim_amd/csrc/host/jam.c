/*
 * jam.c — the jammers on the host: the plain-C statement of csrc/common/gss_jam.h over a range
 * of samples (gss_jam_host), the argument checks it shares with the launch (gss_jam_check), and
 * gss_jam_make, which turns physical parameters into a gss_jam_t once for the CLI and the
 * binding.  The reference has no interference model; like the noise this is an extension applied
 * to its 16-bit samples before the quantise/pack epilogue (gpssim.c:2266-2288).  gss_jam_host is
 * what the GPU kernels (csrc/hip/gss_jam.hip) are tested against.
 */
#include <math.h>
#include <pthread.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_stage.h"
#include "../common/gss_jam.h"

int gss_impair_check(const gss_impair_t *p, const void *iq, uint64_t sample0, size_t n, int fmt,
                     const void *out);                                        /* impair.c */

static uint32_t jam_lut[GSS_JAM_LUT];
static int32_t jam_noise[GSS_IMP_TBL];
static pthread_once_t jam_once = PTHREAD_ONCE_INIT;

static void jam_tables_make(void)
{
    int32_t s[512], c[512];
    gss_lut(s, c);
    for (int i = 0; i < GSS_JAM_LUT; i++)
        jam_lut[i] = gss_jam_cell(c[i], s[i]);
    gss_noise_table(jam_noise);
}

/* the jammers' own argument checks, shared by gss_jam_host and gss_jam_device */
int gss_jam_check(const gss_jam_t *jam, int n_jam)
{
    if (n_jam < 0 || n_jam > GSS_MAXJAM || (n_jam > 0 && !jam))
        return gss_fail(GSS_E_ARG, "invalid jammers (0..%d of them)", GSS_MAXJAM);
    for (int i = 0; i < n_jam; i++) {
        const gss_jam_t *j = &jam[i];
        if (j->sweep == 0 || j->amp > GSS_JAM_AMP_MAX || j->gate_on > j->gate_period ||
            j->gate_shift >= (j->gate_period ? j->gate_period : 1u) || j->pad != 0)
            return gss_fail(GSS_E_ARG, "invalid jammer %d (sweep >= 1, amp <= 2^23, gate_on <= "
                                       "gate_period, gate_shift < max(gate_period, 1), pad 0)", i);
    }
    return 0;
}

int gss_jam_host(const gss_impair_t *p, const gss_jam_t *jam, int n_jam, const int16_t *iq,
                 uint64_t sample0, size_t n, int fmt, void *out)
{
    int rc = gss_impair_check(p, iq, sample0, n, fmt, out);
    if (!rc)
        rc = gss_jam_check(jam, n_jam);
    if (rc)
        return rc;
    pthread_once(&jam_once, jam_tables_make);
    const uint32_t k0 = (uint32_t)p->seed, k1 = (uint32_t)(p->seed >> 32);
    gss_jam_state_t st[GSS_MAXJAM];
    for (int i = 0; i < n_jam; i++)
        gss_jam_seed(&jam[i], sample0, &st[i]);
    uint32_t w[4] = {0, 0, 0, 0};
    uint8_t byte = 0;
    for (size_t j = 0; j < n; j++) {
        const uint64_t a = sample0 + j;
        if (j == 0 || !(a & 1))
            gss_imp_philox((uint32_t)(a >> 1), (uint32_t)(a >> 33), k0, k1, w);
        int32_t jc[2] = {0, 0};
        for (int i = 0; i < n_jam; i++) {
            gss_jam_add(&jam[i], &st[i], jam_lut, &jc[0], &jc[1]);
            gss_jam_next(&jam[i], &st[i]);
        }
        for (int c = 0; c < 2; c++) {
            const int32_t g = gss_imp_noise(w[2 * (a & 1) + c], jam_noise, p->sigma_q8);
            gss_imp_put(out, fmt, 2 * j + c, gss_imp_level(iq[2 * j + c] + jc[c], g, p->shift),
                        &byte);
        }
    }
    return 0;
}

/* floor(f / fs 2^64 + 0.5) as int64; |f| < fs / 2 keeps it inside */
static int jam_step(double f, double fs, int64_t *out)
{
    if (!isfinite(f) || !(fabs(f) < fs / 2.0))
        return 1;
    const double v = floor(f / fs * 18446744073709551616.0 + 0.5);
    if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0))
        return 1;
    *out = (int64_t)v;
    return 0;
}

int gss_jam_make(double fs_hz, double js_db, double f0_hz, double f1_hz, double sweep_s,
                 double gate_period_s, double duty, gss_jam_t *out)
{
    if (!out || !isfinite(fs_hz) || !(fs_hz > 0.0) || !isfinite(js_db) || !isfinite(sweep_s) ||
        sweep_s < 0.0 || !isfinite(gate_period_s) || gate_period_s < 0.0)
        return gss_fail(GSS_E_ARG, "invalid jammer parameters");
    gss_jam_t j;
    memset(&j, 0, sizeof j);
    const double amp = floor(65536.0 * pow(10.0, js_db / 20.0) + 0.5);
    if (!(amp <= (double)GSS_JAM_AMP_MAX))
        return gss_fail(GSS_E_ARG, "jammer level out of range (at most 42.1 dB)");
    j.amp = (uint32_t)amp;
    int64_t s0, s1;
    if (jam_step(f0_hz, fs_hz, &s0))
        return gss_fail(GSS_E_ARG, "jammer frequency outside (-fs/2, fs/2)");
    j.step0 = (uint64_t)s0;
    j.sweep = 1;
    if (sweep_s > 0.0) {
        const double P = floor(sweep_s * fs_hz + 0.5);
        if (!(P >= 1.0 && P <= 4294967295.0))
            return gss_fail(GSS_E_ARG, "jammer sweep outside 1..2^32-1 samples");
        if (jam_step(f1_hz, fs_hz, &s1))
            return gss_fail(GSS_E_ARG, "jammer frequency outside (-fs/2, fs/2)");
        j.sweep = (uint32_t)P;
        /* |s1 - s0| < 2^64: in 128 bits, floored, then mod 2^64 */
        const __int128 d = (__int128)s1 - (__int128)s0, q = d / (__int128)j.sweep;
        j.rate = (uint64_t)(q - ((d % (__int128)j.sweep) < 0 ? 1 : 0));
    }
    if (gate_period_s > 0.0) {
        const double gp = floor(gate_period_s * fs_hz + 0.5);
        if (!(gp >= 1.0 && gp <= 4294967295.0) || !isfinite(duty) || duty < 0.0 || duty > 1.0)
            return gss_fail(GSS_E_ARG, "jammer pulse outside 1..2^32-1 samples, duty 0..1");
        j.gate_period = (uint32_t)gp;
        j.gate_on = (uint32_t)floor(duty * gp + 0.5);
    }
    *out = j;
    return 0;
}
