/*
 * navdata.c — the navigation data a position fix needs (gss_navdata_*, include/gpssim_amd.h;
 * DESIGN.md §15): per PRN one ephemeris in use and the Klobuchar coefficients.  A RINEX file
 * gives every set it holds (rinex_read, the simulator's reader); decoded subframes select among
 * them by IODE or, on a handle opened empty, are decoded themselves: the inverse of
 * nav_subframes (gnss_navmsg.c) with the IS-GPS-200 scale factors.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "gss_host.h"

int gss_navdata_open_empty(gss_navdata **h)
{
    if (!h)
        return gss_fail(GSS_E_ARG, "invalid navdata arguments");
    *h = (gss_navdata *)calloc(1, sizeof **h);
    return *h ? 0 : gss_fail(GSS_E_NOMEM, "out of memory");
}

int gss_navdata_open_rinex(gss_navdata **h, const char *path)
{
    if (!h || !path)
        return gss_fail(GSS_E_ARG, "invalid navdata arguments");
    int rc = gss_navdata_open_empty(h);
    if (rc)
        return rc;
    const int n = rinex_read((*h)->sets, &(*h)->io, path);
    if (n < 1) {
        free(*h);
        *h = NULL;
        return n < 0 ? gss_fail(GSS_E_IO, "navdata: cannot read %s", path)
                     : gss_fail(GSS_E_INPUT, "navdata: no ephemeris in %s", path);
    }
    (*h)->n_sets = n;
    (*h)->io.enable = 1;
    return 0;
}

int gss_navdata_close(gss_navdata *h)
{
    free(h);
    return 0;
}

/* the low `bits` bits of v as a two's-complement number */
static double sx(uint32_t v, int bits)
{
    const uint32_t m = 1u << (bits - 1);
    v &= (m << 1) - 1u;
    return (double)((int64_t)(v ^ m) - (int64_t)m);
}

/* subframes 1-3 of one IODE as an ephemeris (IS-GPS-200 tables 20-I and 20-III) */
static void decode_eph(const gss_navdata *h, int sv, eph_t *e)
{
    const uint32_t *a = h->sf[sv][0], *b = h->sf[sv][1], *c = h->sf[sv][2];
    memset(e, 0, sizeof *e);
    e->iodc = (int)((a[2] & 3u) << 8 | a[7] >> 16);
    e->codeL2 = (int)(a[2] >> 12 & 3u);
    e->svhlth = (int)(a[2] >> 2 & 0x3Fu);
    e->tgd = sx(a[6], 8) * K_P2_M31;
    e->toc.sec = (double)(a[7] & 0xFFFFu) * 16.0;
    e->af2 = sx(a[8] >> 16, 8) * K_P2_M55;
    e->af1 = sx(a[8], 16) * K_P2_M43;
    e->af0 = sx(a[9] >> 2, 22) * K_P2_M31;
    e->iode = (int)(b[2] >> 16);
    e->crs = sx(b[2], 16) * K_P2_M5;
    e->deltan = sx(b[3] >> 8, 16) * K_P2_M43 * K_PI;
    e->m0 = sx((b[3] & 0xFFu) << 24 | b[4], 32) * K_P2_M31 * K_PI;
    e->cuc = sx(b[5] >> 8, 16) * K_P2_M29;
    e->ecc = (double)((b[5] & 0xFFu) << 24 | b[6]) * K_P2_M33;
    e->cus = sx(b[7] >> 8, 16) * K_P2_M29;
    e->sqrta = (double)((b[7] & 0xFFu) << 24 | b[8]) * K_P2_M19;
    e->toe.sec = (double)(b[9] >> 8) * 16.0;
    e->cic = sx(c[2] >> 8, 16) * K_P2_M29;
    e->omg0 = sx((c[2] & 0xFFu) << 24 | c[3], 32) * K_P2_M31 * K_PI;
    e->cis = sx(c[4] >> 8, 16) * K_P2_M29;
    e->inc0 = sx((c[4] & 0xFFu) << 24 | c[5], 32) * K_P2_M31 * K_PI;
    e->crc = sx(c[6] >> 8, 16) * K_P2_M5;
    e->aop = sx((c[6] & 0xFFu) << 24 | c[7], 32) * K_P2_M31 * K_PI;
    e->omgdot = sx(c[8], 24) * K_P2_M43 * K_PI;
    e->idot = sx(c[9] >> 2, 14) * K_P2_M43 * K_PI;
    e->A = e->sqrta * e->sqrta;                              /* as rinex_read derives them */
    e->n = sqrt(K_GM / (e->A * e->A * e->A)) + e->deltan;
    e->sq1e2 = sqrt(1.0 - e->ecc * e->ecc);
    e->omgkdot = e->omgdot - K_OMEGA_E;
    e->vflg = e->sqrta > 0.0;
}

int gss_navdata_add_subframe(gss_navdata *h, int prn, const gss_nav_sf_t *sf)
{
    if (!h || !sf || prn < 1 || prn > K_MAX_SAT || sf->id < 1 || sf->id > 5)
        return gss_fail(GSS_E_ARG, "invalid navdata arguments");
    const int sv = prn - 1;
    uint32_t d[K_N_DWRD_SBF];                                /* the words' 24 data bits */
    d[0] = sf->word[0] >> 6 & 0xFFFFFFu;
    for (int i = 1; i < K_N_DWRD_SBF; i++) {
        const uint32_t w = sf->word[i - 1] & 1u ? ~sf->word[i] : sf->word[i];   /* D30* set */
        d[i] = w >> 6 & 0xFFFFFFu;
    }
    if (sf->id == 4) {
        if ((d[2] >> 16 & 0x3Fu) != 56u)                     /* page 18 alone says something */
            return 0;
        iono_t *io = &h->io;
        if (h->n_sets == 0 || !io->vflg) {
            io->alpha0 = sx(d[2] >> 8, 8) * K_P2_M30;
            io->alpha1 = sx(d[2], 8) * K_P2_M27;
            io->alpha2 = sx(d[3] >> 16, 8) * K_P2_M24;
            io->alpha3 = sx(d[3] >> 8, 8) * K_P2_M24;
            io->beta0 = sx(d[3], 8) * 2048.0;
            io->beta1 = sx(d[4] >> 16, 8) * 16384.0;
            io->beta2 = sx(d[4] >> 8, 8) * 65536.0;
            io->beta3 = sx(d[4], 8) * 65536.0;
            io->vflg = 1;
            io->enable = 1;
        }
        return 0;
    }
    if (sf->id == 5)
        return 0;
    const int k = sf->id - 1;
    memcpy(h->sf[sv][k], d, sizeof d);
    h->have[sv][k] = 1;
    if (k == 0)
        h->wn[sv] = (int)(d[2] >> 14 & 0x3FFu);
    if (h->n_sets > 0) {                                     /* the RINEX set of this IODE */
        if (k == 0)
            return 0;
        const int iode = (int)(k == 1 ? d[2] >> 16 : d[9] >> 16);
        for (int s = 0; s < h->n_sets; s++)
            if (h->sets[s][sv].vflg == 1 && h->sets[s][sv].iode == iode) {
                h->cur[sv] = h->sets[s][sv];
                break;
            }
        return 0;
    }
    if (h->have[sv][0] && h->have[sv][1] && h->have[sv][2]) {
        const uint32_t iode2 = h->sf[sv][1][2] >> 16, iode3 = h->sf[sv][2][9] >> 16;
        const uint32_t iodc = h->sf[sv][0][7] >> 16;
        if (iode2 == iode3 && iode2 == iodc) {
            decode_eph(h, sv, &h->cur[sv]);
            h->cur[sv].toe.week = h->cur[sv].toc.week = h->wn[sv];
        }
    }
    return 0;
}

const eph_t *navdata_eph(const gss_navdata *h, int prn, double sec)
{
    if (prn < 1 || prn > K_MAX_SAT)
        return NULL;
    const int sv = prn - 1;
    if (h->cur[sv].vflg == 1)
        return &h->cur[sv];
    const eph_t *best = NULL;
    double best_dt = 7200.0;                                 /* a set serves two hours */
    for (int s = 0; s < h->n_sets; s++) {
        const eph_t *e = &h->sets[s][sv];
        if (e->vflg != 1)
            continue;
        double dt = sec - e->toc.sec;
        if (dt > K_SEC_HALF_WEEK)
            dt -= K_SEC_WEEK;
        else if (dt < -K_SEC_HALF_WEEK)
            dt += K_SEC_WEEK;
        if (fabs(dt) <= best_dt) {
            best_dt = fabs(dt);
            best = e;
        }
    }
    return best;
}

int gss_navdata_get(const gss_navdata *h, int prn, double *fields, int n)
{
    if (!h || !fields || n < 0 || n > GSS_NAVDATA_FIELDS || prn < 1 || prn > K_MAX_SAT)
        return gss_fail(GSS_E_ARG, "invalid navdata arguments");
    const eph_t *e = &h->cur[prn - 1];
    const double f[GSS_NAVDATA_FIELDS] = {
        e->vflg == 1, e->iode, e->iodc, e->toc.sec, e->toe.sec, e->af0, e->af1, e->af2, e->tgd,
        e->crs, e->deltan, e->m0, e->cuc, e->ecc, e->cus, e->sqrta, e->cic, e->omg0, e->cis,
        e->inc0, e->crc, e->aop, e->omgdot, e->idot, h->io.vflg == 1, h->io.alpha0, h->io.alpha1,
        h->io.alpha2, h->io.alpha3, h->io.beta0, h->io.beta1, h->io.beta2, h->io.beta3,
        e->toe.week};
    memcpy(fields, f, (size_t)n * sizeof *fields);
    return 0;
}
