/*
 * gps-sdr-pvt — does a receiver that plays a file of I/Q samples as gps-sdr-sim writes them come
 * out at the scenario's location and time?  Acquires and tracks as gps-sdr-track does (one
 * window), decodes the subframes, takes the observables at a fixed rate from sample 0 of the
 * range (gss_obs_host) and solves a fix wherever four satellites are past bit synchronisation
 * (gss_pvt_solve).  One line per fix:
 *   FIX k t s sats n x y z [m] lat lon [deg] h [m] speed [m/s] t0 week sec pdop p rms r [m]
 * t0 is the GPS time of sample 0 of the range as the fix sees it.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "cli_rx.h"

#define MAX_SF    64
#define BIT_SKIP  500            /* gss_nav_decode's default: bit synchronisation starts here    */
#define R2D       57.2957795131

static void usage(void)
{
    fprintf(stderr,
        "Usage: gps-sdr-pvt [options]\n"
        "Options:\n"
        "  -f <file>          I/Q sample file (required)\n"
        "  -s <frequency>     Sampling frequency [Hz] (required)\n"
        "  -b <iq_bits>       I/Q data format [1/8/16] (default: 16)\n"
        "  -e <gps_nav>       RINEX navigation file the samples were made from.  Without it the\n"
        "                     fixes need subframes 1-3 from the file itself: about 37 s of signal\n"
        "  -t <seconds>       Start of the range in the file (default: 0)\n"
        "  -d <seconds>       Length of the range (default: to the end of the file)\n"
        "  --rate=<Hz>        Fixes per second, from sample 0 of the range (default: 10)\n"
        "  --prn=<list>       PRNs, e.g. 1,3,7-9 (default: 1-32)\n"
        "  --no-iono          The samples were made with -i (no ionospheric delay)\n"
        "  --host             Search and track on the CPU (no GPU needed); prints the same text\n"
        "  --csv=<file>       Write t,x,y,z of every fix in the format gps-sdr-sim -u reads\n"
        "The observables are taken on the CPU either way: the records are in host memory after\n"
        "tracking, and walking them there is faster than uploading them again.\n");
}

int main(int argc, char **argv)
{
    const char *nav_file = NULL, *csv_file = NULL;
    rx_opts_t o = RX_OPTS_DEFAULT;
    double dur = -1, rate = 10;
    uint32_t mask = 0xFFFFFFFFu;
    int host = 0;
    gss_pvt_opts_t popt = {0, 0};
    if (argc < 2) {
        usage();
        return 1;
    }
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        char *end;
        const int shared = rx_option(argc, argv, &i, &o, usage);
        if (shared < 0)
            return 1;
        if (shared)
            continue;
        if (!strcmp(a, "-d") || !strcmp(a, "-e")) {
            if (i + 1 >= argc) {
                usage();
                return 1;
            }
            if (a[1] == 'e') {
                nav_file = argv[++i];
                continue;
            }
            dur = strtod(argv[++i], &end);
            if (*end || !(dur > 0.0))
                return rx_fail("Invalid duration.");
        } else if (!strncmp(a, "--rate=", 7)) {
            rate = strtod(a + 7, &end);
            if (*end || !(rate > 0.0) || rate > 1000.0)
                return rx_fail("Invalid fix rate (above 0, at most 1000 Hz).");
        } else if (!strncmp(a, "--prn=", 6)) {
            if (rx_parse_prns(a + 6, &mask))
                return rx_fail("Invalid PRN list (1..32, e.g. 1,3,7-9).");
        } else if (!strncmp(a, "--csv=", 6)) {
            csv_file = a + 6;
        } else if (!strcmp(a, "--no-iono")) {
            popt.no_iono = 1;
        } else if (!strcmp(a, "--host")) {
            host = 1;
        } else {
            usage();
            return 1;
        }
    }
    if (rx_required(&o))
        return 1;
    const double fs = o.fs;
    const long bits = o.bits;

    gss_acq_t acq;
    acq.fs_hz = (int32_t)fs;
    acq.fmt = (int32_t)bits;
    acq.coh_ms = 1;
    acq.n_coh = 10;
    acq.bin_hz = 250;
    acq.n_half = 20;
    acq.qshift = -1;
    acq.prn_mask = mask;
    gss_trk_cfg_t cfg;
    int32_t T, n_prn;
    int64_t n_acq;
    if (gss_acq_sizes(&acq, NULL, &T, &n_acq, NULL, &n_prn) ||
        gss_trk_defaults(acq.fs_hz, acq.fmt, &cfg)) {
        fprintf(stderr, "ERROR: %s\n", gss_last_error());
        return 1;
    }
    const int64_t step = (int64_t)floor(fs / rate + 0.5);
    if (step < 1)
        return rx_fail("Invalid fix rate (above the sample rate).");

    FILE *fp = fopen(o.file, "rb");
    if (!fp || fseeko(fp, 0, SEEK_END) != 0)
        return rx_fail("Failed to open the sample file.");
    const int64_t fbytes = (int64_t)ftello(fp);
    const int64_t in_file = bits == 16 ? fbytes / 4 : bits == 8 ? fbytes / 2 : fbytes * 4;
    const int64_t first = rx_first_sample(&o);
    int64_t N = in_file - first;
    if (dur > 0 && (int64_t)floor(dur * fs) < N)
        N = (int64_t)floor(dur * fs);
    if (bits == 1)
        N -= N % 4;
    const int32_t n_epoch = N > T ? (int32_t)((N - T) * 1000 / (int64_t)fs) - 1 : 0;
    if (N < n_acq || n_epoch < 1)
        return rx_fail("The range is too short to acquire and track.");
    void *x = malloc(rx_bytes(bits, N));
    if (!x)
        return rx_fail("Out of memory.");
    if (rx_read(fp, bits, first, N, x)) {
        fclose(fp);
        return rx_fail("Failed to read the sample file.");
    }
    fclose(fp);

    gss_navdata *nd = NULL;
    if (nav_file ? gss_navdata_open_rinex(&nd, nav_file) : gss_navdata_open_empty(&nd)) {
        fprintf(stderr, "ERROR: %s\n", gss_last_error());
        return 1;
    }
    gss_dev *dev = NULL;
    int rc = host ? 0 : gss_dev_open(&dev, 0);
    const double thr = gss_acq_threshold(acq.n_coh, (uint64_t)(2 * acq.n_half + 1) * (uint64_t)T,
                                         1e-3);
    gss_acq_peak_t *peaks = (gss_acq_peak_t *)calloc((size_t)n_prn, sizeof *peaks);
    gss_trk_job_t *jobs = (gss_trk_job_t *)calloc((size_t)n_prn, sizeof *jobs);
    if (!peaks || !jobs)
        return rx_fail("Out of memory.");
    int n_job = 0;
    if (rc == 0)
        rc = host ? gss_acquire_host(&acq, x, peaks, NULL, NULL, 16)
                  : gss_acquire(dev, &acq, x, peaks, NULL, NULL);
    for (int p = 0; p < n_prn && rc == 0; p++)
        if (rx_peak_ratio(&peaks[p]) >= thr)
            rc = gss_trk_job_from_peak(&acq, &peaks[p], 0, n_epoch, &jobs[n_job++]);
    gss_trk_rec_t *rec = NULL;
    int32_t *count = NULL;
    if (rc == 0 && n_job > 0) {
        rec = (gss_trk_rec_t *)malloc((size_t)n_job * n_epoch * sizeof *rec);
        count = (int32_t *)calloc((size_t)n_job, sizeof *count);
        if (!rec || !count)
            return rx_fail("Out of memory.");
        rc = host ? gss_track_host(&cfg, x, N, jobs, n_job, rec, n_epoch, count, 16)
                  : gss_track(dev, &cfg, x, N, jobs, n_job, rec, n_epoch, count);
    }
    if (dev)
        gss_dev_close(dev);
    free(x);

    /* per job: its subframes into the navigation data, the first as the anchor, and the epoch
       from which its bits are synchronised */
    const int32_t n_fix = (int32_t)((N - 1) / step + 1);
    gss_obs_t *obs = NULL;
    gss_pvt_sat_t *sats = (gss_pvt_sat_t *)calloc((size_t)(n_job ? n_job : 1), sizeof *sats);
    gss_nav_sf_t *anchor = (gss_nav_sf_t *)calloc((size_t)(n_job ? n_job : 1), sizeof *anchor);
    int32_t *ready = (int32_t *)calloc((size_t)(n_job ? n_job : 1), sizeof *ready);
    if (!sats || !anchor || !ready)
        return rx_fail("Out of memory.");
    for (int j = 0; j < n_job && rc == 0; j++) {
        gss_nav_sf_t sf[MAX_SF];
        int32_t off = 0;
        const int n_sf = gss_nav_decode(rec + (size_t)j * n_epoch, count[j], -1, sf, MAX_SF, &off);
        if (n_sf < 0)
            rc = n_sf;
        for (int k = 0; k < n_sf && rc == 0; k++)
            rc = gss_navdata_add_subframe(nd, jobs[j].prn, &sf[k]);
        ready[j] = n_sf > 0 ? BIT_SKIP + off : -1;
        if (n_sf > 0)
            anchor[j] = sf[0];
    }
    if (rc == 0 && n_job > 0) {
        obs = (gss_obs_t *)malloc((size_t)n_job * n_fix * sizeof *obs);
        if (!obs)
            return rx_fail("Out of memory.");
        rc = gss_obs_host(acq.fs_hz, rec, n_epoch, count, n_job, 0, step, n_fix, obs, 16);
    }
    if (rc) {
        fprintf(stderr, "ERROR: %s\n", gss_last_error());
        return 1;
    }
    fprintf(stderr, "Range: %lld samples from %lld, %d epochs; %d satellite(s), %d instant(s)\n",
            (long long)N, (long long)first, n_epoch, n_job, n_fix);

    FILE *cf = csv_file ? fopen(csv_file, "w") : NULL;
    if (csv_file && !cf)
        return rx_fail("Failed to open the csv file.");
    int n_out = 0;
    for (int32_t k = 0; k < n_fix; k++) {
        int n = 0;
        for (int j = 0; j < n_job; j++) {
            const gss_obs_t *ob = &obs[(size_t)j * n_fix + k];
            if (ready[j] < 0 || ob->epoch < ready[j])
                continue;
            sats[n].obs = *ob;
            sats[n].prn = jobs[j].prn;
            sats[n].sf_epoch = anchor[j].epoch;
            sats[n].sf_tow = anchor[j].tow;
            n++;
        }
        if (n < 4)
            continue;
        gss_pvt_fix_t fix;
        if (gss_pvt_solve(nd, fs, (int64_t)k * step, sats, n, &popt, &fix)) {
            fprintf(stderr, "ERROR: %s\n", gss_last_error());
            return 1;
        }
        if (fix.status != GSS_PVT_OK)
            continue;
        const double t = (double)k * (double)step / fs;
        const double v = sqrt(fix.vel[0] * fix.vel[0] + fix.vel[1] * fix.vel[1] +
                              fix.vel[2] * fix.vel[2]);
        printf("FIX %d t %.3f sats %d %.3f %.3f %.3f %.7f %.7f %.2f speed %.3f t0 %d %.9f "
               "pdop %.2f rms %.2f\n", k, t, fix.n_used, fix.xyz[0], fix.xyz[1], fix.xyz[2],
               fix.llh[0] * R2D, fix.llh[1] * R2D, fix.llh[2], v, fix.t0_week, fix.t0_sec,
               fix.pdop, fix.rms);
        if (cf)
            fprintf(cf, "%5.1f,%12.3f,%12.3f,%12.3f\n", t, fix.xyz[0], fix.xyz[1], fix.xyz[2]);
        n_out++;
    }
    if (cf)
        fclose(cf);
    if (n_out == 0)
        fprintf(stderr, "No fix: fewer than four satellites with an ephemeris.\n");
    gss_navdata_close(nd);
    free(peaks);
    free(jobs);
    free(rec);
    free(count);
    free(obs);
    free(sats);
    free(anchor);
    free(ready);
    return 0;
}
