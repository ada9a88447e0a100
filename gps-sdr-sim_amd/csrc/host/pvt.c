/*
 * pvt.c — the position fix from observables (gss_pvt_solve, include/gpssim_amd.h; DESIGN.md
 * §15).  Double arithmetic on the host: libm cannot be matched bit for bit on a GPU (DESIGN.md
 * §9), and a fix is a few thousand operations.
 *
 * The fix inverts the simulator's own range model (sv_range_at, gnss_orbit.c): what a rendered
 * file encodes is that model's pseudorange at the receive time, so a wrong sign anywhere in it
 * (ionosphere, clock, Sagnac rotation) moves the fix.  Times are kept as a whole second plus a
 * fraction: a second of week near 6e5 is a double with 2^-33 s (3.5 cm of range) between
 * neighbours, and only the satellites' motion (below 1 km/s) may see that rounding.
 */
#include <math.h>
#include <string.h>
#include "gss_host.h"
#include "../common/gss_trk.h"

#define PVT_MAX_SAT   K_MAX_SAT
#define PVT_MAX_ITER  30
#define PVT_TOL       1.0e-6         /* [m]: a step below it ends the iteration                  */

/* n[4][4] -> its inverse by Gauss-Jordan with partial pivoting; 0, or -1 when singular */
static int invert4(double n[4][4], double inv[4][4])
{
    double a[4][8];
    double scale = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            a[i][j] = n[i][j];
            a[i][4 + j] = i == j;
            if (fabs(n[i][j]) > scale)
                scale = fabs(n[i][j]);
        }
    if (!(scale > 0.0) || !isfinite(scale))
        return -1;
    for (int c = 0; c < 4; c++) {
        int p = c;
        for (int i = c + 1; i < 4; i++)
            if (fabs(a[i][c]) > fabs(a[p][c]))
                p = i;
        if (!(fabs(a[p][c]) > 1.0e-10 * scale))
            return -1;
        for (int j = 0; j < 8; j++) {
            const double t = a[c][j];
            a[c][j] = a[p][j];
            a[p][j] = t;
        }
        const double d = a[c][c];
        for (int j = 0; j < 8; j++)
            a[c][j] /= d;
        for (int i = 0; i < 4; i++) {
            if (i == c)
                continue;
            const double f = a[i][c];
            for (int j = 0; j < 8; j++)
                a[i][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            inv[i][j] = a[i][4 + j];
    return 0;
}

/* the model at receive time g and position xyz: pseudorange, its rate (clock drift included, as
   the difference of two ranges holds it) and the unit vector towards the satellite */
static void model(const eph_t *e, const iono_t *io, gtime_t g, const double *xyz, double *range,
                  double *rate, double *u)
{
    double llh[3], tmat[3][3], pos[3], vel[3], clk[2];
    rng_t rho;
    ecef_to_llh(xyz, llh);
    enu_matrix(llh, tmat);
    sv_range_at(&rho, e, io, g, xyz, llh, tmat);
    sv_state(e, g, pos, vel, clk);
    *range = rho.range;
    *rate = rho.rate - K_C * clk[1];
    const double ce = cos(rho.azel[1]);
    const double neu[3] = {ce * cos(rho.azel[0]), ce * sin(rho.azel[0]), sin(rho.azel[1])};
    for (int i = 0; i < 3; i++)
        u[i] = tmat[0][i] * neu[0] + tmat[1][i] * neu[1] + tmat[2][i] * neu[2];
}

int gss_pvt_range(const gss_navdata *h, int prn, int week, double sec, const double *xyz,
                  int no_iono, double *out)
{
    if (!h || !xyz || !out || prn < 1 || prn > K_MAX_SAT)
        return gss_fail(GSS_E_ARG, "invalid fix arguments");
    const eph_t *e = navdata_eph(h, prn, sec);
    if (!e)
        return gss_fail(GSS_E_STATE, "no ephemeris for PRN %d", prn);
    iono_t io = h->io;
    if (no_iono)
        io.enable = 0;
    const gtime_t g = {week, sec};
    double u[3];
    model(e, &io, g, xyz, &out[0], &out[1], u);
    return 0;
}

int gss_pvt_solve(const gss_navdata *h, double fs, int64_t t, const gss_pvt_sat_t *sats, int n_sat,
                  const gss_pvt_opts_t *opts, gss_pvt_fix_t *out)
{
    if (!h || !out || !(fs >= 1.0) || n_sat < 0 || (n_sat > 0 && !sats) || t < 0 ||
        t > GSS_TRK_S0MAX)
        return gss_fail(GSS_E_ARG, "invalid fix arguments");
    memset(out, 0, sizeof *out);
    out->status = GSS_PVT_FEW;

    /* transmit times as a whole second and a fraction of one */
    const eph_t *eph[PVT_MAX_SAT];
    int64_t tx_i[PVT_MAX_SAT];
    double tx_f[PVT_MAX_SAT], w[PVT_MAX_SAT];
    int n = 0, week = opts ? opts->week : 0;
    for (int i = 0; i < n_sat && n < PVT_MAX_SAT; i++) {
        const gss_pvt_sat_t *s = &sats[i];
        if (s->obs.epoch < 0 || s->prn < 1 || s->prn > K_MAX_SAT || s->sf_tow < 0 ||
            s->obs.code < 0 || s->obs.code >= GSS_TRK_M)
            continue;
        const int64_t de = (int64_t)s->obs.epoch - s->sf_epoch;
        int64_t q = de / 1000, r = de % 1000;
        if (r < 0) {
            r += 1000;
            q--;
        }
        const int64_t sec = 6 * ((int64_t)s->sf_tow - 1) + q;
        const eph_t *e = navdata_eph(h, s->prn, (double)sec);
        if (!e)
            continue;
        eph[n] = e;
        tx_i[n] = sec;
        tx_f[n] = ((double)r + (double)s->obs.code / (double)GSS_TRK_M) * 1e-3;
        w[n] = (double)s->obs.w;
        if (week == 0)
            week = e->toe.week;
        n++;
    }
    out->n_used = n;
    if (n < 4)
        return 0;

    iono_t io = h->io, io_off = h->io;
    io_off.enable = 0;
    if ((opts && opts->no_iono) || !io.vflg)
        io.enable = 0;
    const double ts = floor((double)t / fs), tf = ((double)t - ts * fs) / fs;
    int64_t tref = tx_i[0];
    for (int i = 1; i < n; i++)
        tref = tx_i[i] < tref ? tx_i[i] : tref;
    /* unknowns: xyz and b = T0 + ts - tref, the receive time being tref + b + tf */
    double xyz[3] = {0.0, 0.0, 0.0}, b = 0.0;
    for (int i = 0; i < n; i++) {
        const double v = (double)(tx_i[i] - tref) + tx_f[i] - tf + 0.075;
        b = (i == 0 || v > b) ? v : b;
    }
    double u[PVT_MAX_SAT][3], res[PVT_MAX_SAT], rate[PVT_MAX_SAT], inv[4][4];
    int it, settled = 0;
    for (it = 0; it < PVT_MAX_ITER; it++) {
        const gtime_t g = {week, (double)tref + (b + tf)};
        const int near = vnorm3(xyz) > 6.0e6;               /* no ionosphere from the earth's core */
        double N[4][4] = {{0}}, y[4] = {0};
        for (int i = 0; i < n; i++) {
            double range;
            model(eph[i], near ? &io : &io_off, g, xyz, &range, &rate[i], u[i]);
            res[i] = K_C * ((double)(tref - tx_i[i]) + (b + tf - tx_f[i])) - range;
            const double row[4] = {u[i][0], u[i][1], u[i][2], 1.0 - rate[i] / K_C};
            for (int a = 0; a < 4; a++) {
                y[a] += row[a] * res[i];
                for (int c = 0; c < 4; c++)
                    N[a][c] += row[a] * row[c];
            }
        }
        if (settled)
            break;
        if (invert4(N, inv) != 0) {
            out->status = GSS_PVT_SINGULAR;
            return 0;
        }
        double d[4];
        for (int a = 0; a < 4; a++)
            d[a] = -(inv[a][0] * y[0] + inv[a][1] * y[1] + inv[a][2] * y[2] + inv[a][3] * y[3]);
        for (int a = 0; a < 3; a++)
            xyz[a] += d[a];
        b += d[3] / K_C;
        if (!isfinite(d[0] + d[1] + d[2] + d[3])) {
            out->status = GSS_PVT_DIVERGED;
            return 0;
        }
        settled = near && vnorm3(d) < PVT_TOL && fabs(d[3]) < PVT_TOL;
    }
    out->iterations = it;
    if (!settled) {
        out->status = GSS_PVT_DIVERGED;
        return 0;
    }

    /* the residuals and geometry of the last evaluation */
    double ss = 0.0;
    for (int i = 0; i < n; i++)
        ss += res[i] * res[i];
    out->rms = sqrt(ss / n);
    out->pdop = sqrt(inv[0][0] + inv[1][1] + inv[2][2]);

    /* velocity and drift: -lambda D_i = rate_i - u_i . v + c drift */
    double N[4][4] = {{0}}, y[4] = {0}, vinv[4][4];
    for (int i = 0; i < n; i++) {
        const double dop = w[i] * fs / 4294967296.0;
        const double m = -K_LAMBDA_L1 * dop - rate[i];
        const double row[4] = {-u[i][0], -u[i][1], -u[i][2], 1.0};
        for (int a = 0; a < 4; a++) {
            y[a] += row[a] * m;
            for (int c = 0; c < 4; c++)
                N[a][c] += row[a] * row[c];
        }
    }
    if (invert4(N, vinv) != 0) {
        out->status = GSS_PVT_SINGULAR;
        return 0;
    }
    for (int a = 0; a < 3; a++)
        out->vel[a] = vinv[a][0] * y[0] + vinv[a][1] * y[1] + vinv[a][2] * y[2] + vinv[a][3] * y[3];
    out->drift = (vinv[3][0] * y[0] + vinv[3][1] * y[1] + vinv[3][2] * y[2] + vinv[3][3] * y[3]) /
                 K_C;

    memcpy(out->xyz, xyz, sizeof xyz);
    ecef_to_llh(xyz, out->llh);
    double fl = (double)tref - ts, fr = b;                  /* T0 = tref - ts + b */
    const double carry = floor(fr);
    fl += carry;
    fr -= carry;
    while (fl < 0.0) {
        fl += K_SEC_WEEK;
        week--;
    }
    while (fl >= K_SEC_WEEK) {
        fl -= K_SEC_WEEK;
        week++;
    }
    out->t0_floor = fl;
    out->t0_frac = fr;
    out->t0_sec = fl + fr;
    out->t0_week = week;
    out->status = GSS_PVT_OK;
    return 0;
}
