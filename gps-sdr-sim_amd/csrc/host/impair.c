/*
 * impair.c — the additive-noise impairment on the host: the table of the half-normal inverse
 * CDF and the plain-C statement of csrc/common/gss_impair.h over a range of samples.  The
 * reference has no noise model; this is an extension applied to its 16-bit samples before the
 * quantise/pack epilogue (gpssim.c:2266-2288).  gss_impair_host is what the GPU kernels
 * (csrc/hip/gss_impair.hip) are tested against, and what a CPU build of gss_run links.
 */
#include <math.h>
#include <pthread.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_stage.h"

/* The standard normal quantile: Wichura, "Algorithm AS241: The Percentage Points of the Normal
   Distribution", Applied Statistics 37 (1988), routine PPND16 (relative error ~1e-16).  Only
   p > 0.5 is asked for here. */
static double normal_quantile(double p)
{
    const double q = p - 0.5;
    double r, num, den;
    if (fabs(q) <= 0.425) {
        r = 0.180625 - q * q;
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r +
                   6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
               1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r +
                   3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
               4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r +
                   2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
                 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
               4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r +
                   1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
               2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r +
                   1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
               5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r +
                   1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
               5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

static int32_t noise_tbl[GSS_IMP_TBL];
static pthread_once_t noise_once = PTHREAD_ONCE_INIT;

/* T[i] = round(2^16 * quantile(0.5 + i / 8192)), the last cell closed at 1 - 2^-15 (4.009 sigma) */
static void noise_tbl_make(void)
{
    for (int i = 0; i < GSS_IMP_TBL - 1; i++)
        noise_tbl[i] = (int32_t)floor(65536.0 * normal_quantile(0.5 + i / 8192.0) + 0.5);
    noise_tbl[GSS_IMP_TBL - 1] =
        (int32_t)floor(65536.0 * normal_quantile(1.0 - 1.0 / 32768.0) + 0.5);
}

int gss_noise_table(int32_t *out)
{
    if (!out)
        return gss_fail(GSS_E_ARG, "invalid noise-table arguments");
    pthread_once(&noise_once, noise_tbl_make);
    memcpy(out, noise_tbl, sizeof noise_tbl);
    return 0;
}

/* the argument checks gss_impair_host and gss_impair_device share (impair.c, gss_impair.hip) */
int gss_impair_check(const gss_impair_t *p, const void *iq, uint64_t sample0, size_t n, int fmt,
                     const void *out)
{
    if (!p || p->sigma_q8 > 0x00FFFFFFu || p->shift < 0 || p->shift > 8)
        return gss_fail(GSS_E_ARG, "invalid impairment (sigma_q8 <= 0xFFFFFF, shift 0..8)");
    if (fmt != GSS_FMT_SC01 && fmt != GSS_FMT_SC08 && fmt != GSS_FMT_SC16)
        return gss_fail(GSS_E_ARG, "invalid format %d", fmt);
    if (fmt == GSS_FMT_SC01 && n % 4 != 0)
        return gss_fail(GSS_E_ARG, "SC01 needs a multiple of 4 samples, not %zu", n);
    if (sample0 + n < sample0 || n > SIZE_MAX / 4)
        return gss_fail(GSS_E_ARG, "sample range past 2^64");
    if (n == 0)
        return 0;
    if (!iq || !out || ((uintptr_t)iq & 1) || (fmt == GSS_FMT_SC16 && ((uintptr_t)out & 1)))
        return gss_fail(GSS_E_ARG, "invalid impairment buffers");
    /* in place for SC16 only; any other overlap would read samples already overwritten */
    const uintptr_t a = (uintptr_t)iq, b = (uintptr_t)out;
    const size_t nb = gss_fmt_bytes(n, fmt);
    if (a < b + nb && b < a + n * 4 && !(fmt == GSS_FMT_SC16 && a == b))
        return gss_fail(GSS_E_ARG, "impairment output overlaps its input (in place: SC16 only)");
    return 0;
}

int gss_impair_host(const gss_impair_t *p, const int16_t *iq, uint64_t sample0, size_t n,
                    int fmt, void *out)
{
    const int rc = gss_impair_check(p, iq, sample0, n, fmt, out);
    if (rc)
        return rc;
    pthread_once(&noise_once, noise_tbl_make);
    const uint32_t k0 = (uint32_t)p->seed, k1 = (uint32_t)(p->seed >> 32);
    uint32_t w[4] = {0, 0, 0, 0};
    uint8_t byte = 0;
    for (size_t j = 0; j < n; j++) {
        const uint64_t a = sample0 + j;
        if (j == 0 || !(a & 1))
            gss_imp_philox((uint32_t)(a >> 1), (uint32_t)(a >> 33), k0, k1, w);
        for (int c = 0; c < 2; c++) {
            const int32_t g = gss_imp_noise(w[2 * (a & 1) + c], noise_tbl, p->sigma_q8);
            gss_imp_put(out, fmt, 2 * j + c, gss_imp_level(iq[2 * j + c], g, p->shift), &byte);
        }
    }
    return 0;
}
