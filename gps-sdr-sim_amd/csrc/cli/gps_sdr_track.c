/*
 * gps-sdr-track — can a receiver stay locked on a file of I/Q samples as gps-sdr-sim writes
 * them, and read the navigation message?  Acquires at the start of the range (gss_acquire_*: 1 ms
 * x 10 windows, 250 Hz bins), tracks every PRN over the search threshold (gss_track_*) and decodes
 * its subframes (gss_nav_decode).  One line per PRN and window:
 *   PRN p window k epochs n lock 0|1 cn0 dB-Hz doppler Hz bit offset subframes m
 * and one per subframe:
 *   SF p window k sample i tow t id s
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "cli_rx.h"

#define LOCK_CN0  28.0           /* tracked C/N0 [dB-Hz] at or above which the line says lock 1  */
#define MAX_SF    64

static void usage(void)
{
    fprintf(stderr,
        "Usage: gps-sdr-track [options]\n"
        "Options:\n"
        "  -f <file>          I/Q sample file (required)\n"
        "  -s <frequency>     Sampling frequency [Hz] (required)\n"
        "  -b <iq_bits>       I/Q data format [1/8/16] (default: 16)\n"
        "  -t <seconds>       Start of the range in the file (default: 0)\n"
        "  -d <seconds>       Length of the range (default: to the end of the file)\n"
        "  --prn=<list>       PRNs, e.g. 1,3,7-9 (default: 1-32)\n"
        "  --fmax=<Hz>        Doppler search range +- (default: 5000)\n"
        "  --host             Search and track on the CPU (no GPU needed); prints the same text\n"
        "  --split=<seconds>  Cut the range into windows of this length; each is acquired and\n"
        "                     tracked on its own and reported on its own lines (the jobs of one\n"
        "                     GPU call are then PRNs x windows).  A subframe that straddles a\n"
        "                     cut is lost, and so is what follows a cut until the loops and the\n"
        "                     bit synchronisation have settled (about 0.5 s).\n"
        "  --records=<file>   Write the tracking records (64 bytes per epoch), job after job in\n"
        "                     the order of the PRN lines\n"
        "lock is 1 when the tracked C/N0 is at least 28 dB-Hz.\n");
}

int main(int argc, char **argv)
{
    const char *rec_file = NULL;
    rx_opts_t o = RX_OPTS_DEFAULT;
    double dur = -1, split = 0;
    long fmax = 5000;
    uint32_t mask = 0xFFFFFFFFu;
    int host = 0;
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
        if (!strcmp(a, "-d")) {
            if (i + 1 >= argc) {
                usage();
                return 1;
            }
            dur = strtod(argv[++i], &end);
            if (*end || !(dur > 0.0))
                return rx_fail("Invalid duration.");
        } else if (!strncmp(a, "--prn=", 6)) {
            if (rx_parse_prns(a + 6, &mask))
                return rx_fail("Invalid PRN list (1..32, e.g. 1,3,7-9).");
        } else if (!strncmp(a, "--fmax=", 7)) {
            fmax = strtol(a + 7, &end, 10);
            if (*end || fmax < 0 || fmax > 1000000)
                return rx_fail("Invalid Doppler range.");
        } else if (!strncmp(a, "--split=", 8)) {
            split = strtod(a + 8, &end);
            if (*end || !(split > 0.0))
                return rx_fail("Invalid window length.");
        } else if (!strncmp(a, "--records=", 10)) {
            rec_file = a + 10;
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
    acq.n_half = (int32_t)(fmax / 250);
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

    /* the range: SC01 packs four samples to a byte, so its start and its windows round down */
    FILE *fp = fopen(o.file, "rb");
    if (!fp || fseeko(fp, 0, SEEK_END) != 0)
        return rx_fail("Failed to open the sample file.");
    const int64_t fbytes = (int64_t)ftello(fp);
    const int64_t in_file = bits == 16 ? fbytes / 4 : bits == 8 ? fbytes / 2 : fbytes * 4;
    const int64_t first = rx_first_sample(&o);
    int64_t N = in_file - first;
    if (dur > 0 && (int64_t)floor(dur * fs) < N)
        N = (int64_t)floor(dur * fs);
    int64_t win = split > 0 ? (int64_t)floor(split * fs) : N;
    if (bits == 1)
        win -= win % 4;
    const int32_t n_epoch = win > T ? (int32_t)((win - T) * 1000 / (int64_t)fs) - 1 : 0;
    if (N < 1 || win < n_acq || win > N || n_epoch < 1)
        return rx_fail("The range or the window is too short to acquire and track.");
    const int n_win = (int)(N / win);
    N = (int64_t)n_win * win;
    void *x = malloc(rx_bytes(bits, N));
    if (!x)
        return rx_fail("Out of memory.");
    if (rx_read(fp, bits, first, N, x)) {
        fclose(fp);
        return rx_fail("Failed to read the sample file.");
    }
    fclose(fp);

    gss_dev *dev = NULL;
    int rc = host ? 0 : gss_dev_open(&dev, 0);
    const size_t nbin = (size_t)(2 * acq.n_half + 1);
    const double thr = gss_acq_threshold(acq.n_coh, (uint64_t)nbin * (uint64_t)T, 1e-3);
    gss_acq_peak_t *peaks = (gss_acq_peak_t *)calloc((size_t)n_prn, sizeof *peaks);
    gss_trk_job_t *jobs = (gss_trk_job_t *)calloc((size_t)n_win * n_prn, sizeof *jobs);
    int *job_win = (int *)calloc((size_t)n_win * n_prn, sizeof *job_win);
    if (!peaks || !jobs || !job_win)
        return rx_fail("Out of memory.");
    int n_job = 0;
    for (int k = 0; k < n_win && rc == 0; k++) {
        const int64_t w0 = (int64_t)k * win;
        const void *xw = (const char *)x + rx_offset(bits, w0);
        rc = host ? gss_acquire_host(&acq, xw, peaks, NULL, NULL, 16)
                  : gss_acquire(dev, &acq, xw, peaks, NULL, NULL);
        for (int p = 0; p < n_prn && rc == 0; p++) {
            if (rx_peak_ratio(&peaks[p]) < thr)
                continue;
            rc = gss_trk_job_from_peak(&acq, &peaks[p], w0, n_epoch, &jobs[n_job]);
            job_win[n_job++] = k;
        }
    }
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
    if (rc) {
        fprintf(stderr, "ERROR: %s\n", gss_last_error());
        return 1;
    }
    fprintf(stderr, "Range: %lld samples from %lld in %d window(s), %d epochs each; %d job(s)\n",
            (long long)N, (long long)first, n_win, n_epoch, n_job);

    FILE *rf = rec_file ? fopen(rec_file, "wb") : NULL;
    if (rec_file && !rf)
        return rx_fail("Failed to open the records file.");
    for (int j = 0; j < n_job; j++) {
        const gss_trk_rec_t *r = rec + (size_t)j * n_epoch;
        gss_nav_sf_t sf[MAX_SF];
        int32_t off = 0;
        const int n_sf = gss_nav_decode(r, count[j], -1, sf, MAX_SF, &off);
        if (n_sf < 0) {
            fprintf(stderr, "ERROR: %s\n", gss_last_error());
            return 1;
        }
        const double cn0 = gss_trk_cn0(r, count[j], count[j] > 500 ? 500 : 0);
        const double dop = count[j] ? (double)r[count[j] - 1].w * fs / 4294967296.0 : 0.0;
        printf("PRN %2d window %d epochs %d lock %d cn0 %.2f doppler %.1f bit %d subframes %d\n",
               jobs[j].prn, job_win[j], count[j], cn0 >= LOCK_CN0, cn0, dop, off, n_sf);
        for (int k = 0; k < n_sf; k++)
            printf("SF %2d window %d sample %lld tow %d id %d\n", jobs[j].prn, job_win[j],
                   (long long)(first + sf[k].sample), sf[k].tow, sf[k].id);
        if (rf && fwrite(r, sizeof *r, (size_t)count[j], rf) != (size_t)count[j])
            return rx_fail("Failed to write the records file.");
    }
    if (rf)
        fclose(rf);
    free(x);
    free(peaks);
    free(jobs);
    free(job_win);
    free(rec);
    free(count);
    return 0;
}
