/*
 * fir.c — the front-end band-limit filter on the host: the plain-C statement of
 * csrc/common/gss_fir.h over a range of SC16 samples (gss_fir_host), the checks it shares with
 * the launch (gss_fir_check, gss_fir_args), and gss_fir_make, which designs the taps once for the
 * CLI and the binding.  The reference has no front-end filter; like the noise, the jammers and the
 * echoes this is an extension applied to its 16-bit samples before the quantise/pack epilogue
 * (gpssim.c:2266-2288).  gss_fir_host is what the GPU kernels (csrc/hip/gss_fir.hip) are tested
 * against, and what a CPU build of gss_run links.
 */
#include <math.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_fir.h"
#include "../common/gss_stage.h"

int gss_fir_check(const gss_fir_t *fir)
{
    if (!fir || gss_fir_invalid(fir))
        return gss_fail(GSS_E_ARG, "invalid filter (1..%d taps, pad 0, sum |taps| <= %d)",
                        GSS_MAXTAP, GSS_FIR_L1_MAX);
    return 0;
}

/* the checks of gss_fir_host and gss_fir_device on what the host can see */
int gss_fir_args(const gss_fir_t *fir, const void *in, const void *halo, size_t n, int fmt,
                 const void *out)
{
    const int rc = gss_fir_check(fir);
    if (rc)
        return rc;
    if (fmt != GSS_FMT_SC01 && fmt != GSS_FMT_SC08 && fmt != GSS_FMT_SC16)
        return gss_fail(GSS_E_ARG, "invalid format %d", fmt);
    if (fmt == GSS_FMT_SC01 && n % 4 != 0)
        return gss_fail(GSS_E_ARG, "SC01 needs a multiple of 4 samples, not %zu", n);
    if (n > SIZE_MAX / 8)
        return gss_fail(GSS_E_ARG, "sample range past 2^64");
    if (n == 0)
        return 0;
    if (!in || !out || ((uintptr_t)in & 1) || ((uintptr_t)halo & 1) ||
        (fmt == GSS_FMT_SC16 && ((uintptr_t)out & 1)))
        return gss_fail(GSS_E_ARG, "invalid filter buffers");
    /* out of place: an output sample is read again by the T - 1 outputs after it */
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    const size_t nb = gss_fmt_bytes(n, fmt);
    if (a < b + nb && b < a + n * 4)
        return gss_fail(GSS_E_ARG, "filter output overlaps its input");
    const uintptr_t h = (uintptr_t)halo;
    if (halo && h < b + nb && b < h + 4 * (size_t)(fir->n_taps - 1))
        return gss_fail(GSS_E_ARG, "filter output overlaps its halo");
    return 0;
}

int gss_fir_host(const gss_fir_t *fir, const int16_t *in, const int16_t *halo, size_t n, int fmt,
                 void *out)
{
    const int rc = gss_fir_args(fir, in, halo, n, fmt, out);
    if (rc)
        return rc;
    const int T = fir->n_taps;
    uint8_t byte = 0;
    for (size_t j = 0; j < n; j++)
        for (int c = 0; c < 2; c++) {
            int32_t acc = 0;
            for (int k = 0; k < T; k++)
                acc += (int32_t)fir->taps[k] * gss_fir_x(in, halo, T, (int64_t)j - k, c);
            gss_imp_put(out, fmt, 2 * j + c, gss_fir_round(acc), &byte);
        }
    return 0;
}

int gss_fir_make(double fs_hz, double bw_hz, int n_taps, gss_fir_t *out)
{
    if (!out || !isfinite(fs_hz) || !isfinite(bw_hz) || !(fs_hz > 0.0) || !(bw_hz > 0.0) ||
        bw_hz > fs_hz || n_taps < 3 || n_taps > 63 || n_taps % 2 == 0)
        return gss_fail(GSS_E_ARG, "invalid filter parameters (0 < bw_hz <= fs_hz, an odd number "
                                   "of taps in 3..63)");
    const double pi = 3.14159265358979323846;
    const int M = n_taps - 1;
    const double c = bw_hz / fs_hz;
    double d[GSS_MAXTAP], S = 0.0;
    for (int k = 0; k <= M; k++) {
        const int m = k - M / 2;
        const double s = m == 0 ? c : sin(pi * c * (double)m) / (pi * (double)m);
        d[k] = s * (0.54 - 0.46 * cos(2.0 * pi * (double)k / (double)M));
    }
    for (int k = 0; k <= M; k++)
        S += d[k];
    gss_fir_t f;
    memset(&f, 0, sizeof f);
    f.n_taps = n_taps;
    int32_t sum = 0;
    for (int k = 0; k <= M; k++) {
        const double t = floor(d[k] / S * 16384.0 + 0.5);
        if (!(t >= -32768.0 && t <= 32767.0))
            return gss_fail(GSS_E_ARG, "filter tap %d out of range", k);
        f.taps[k] = (int16_t)t;
        sum += f.taps[k];
    }
    const int32_t centre = (int32_t)f.taps[M / 2] + 16384 - sum;
    if (centre < -32768 || centre > 32767)
        return gss_fail(GSS_E_ARG, "filter centre tap out of range");
    f.taps[M / 2] = (int16_t)centre;
    const int rc = gss_fir_check(&f);
    if (rc)
        return rc;
    *out = f;
    return 0;
}
